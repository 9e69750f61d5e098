"""Hand-made label maps for the region-graph tests, and the run that both the tests and their child processes share."""
import hashlib

import numpy as np


def blocks(h, w, bh, bw):
    """bh x bw blocks in raster order, clipped at the right and bottom edges."""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy // bh) * ((w + bw - 1) // bw) + xx // bw).astype(np.int32)


def hub(h=48, w=64):
    """One background region (label 0) around a 5 x 7 grid of 4 x 4 blocks: the hub has 35 neighbours."""
    seg = np.zeros((h, w), np.int32)
    for r in range(5):
        for c in range(7):
            y, x = 4 + r * 8, 4 + c * 8
            seg[y:y + 4, x:x + 4] = 1 + r * 7 + c
    return seg


def stripes(h, w, vertical):
    yy, xx = np.mgrid[0:h, 0:w]
    return (xx if vertical else yy).astype(np.int32)


def bands(h, w, n):
    """n vertical bands of nearly equal width."""
    return np.broadcast_to((np.arange(w) * n // w).astype(np.int32), (h, w)).copy()


def scattered(h, w, n, seed):
    """Every pixel draws one of n labels: far more distinct adjacent pairs than a planar map of n regions has."""
    rng = np.random.default_rng(seed)
    seg = rng.integers(0, n, (h, w)).astype(np.int32)
    seg.flat[:n] = np.arange(n)                       # every label is present
    return seg


def ragged_batch():
    """Label maps of very different N at one size (48 x 64), for one batch."""
    h, w = 48, 64
    return [hub(h, w), stripes(h, w, True), np.zeros((h, w), np.int32), stripes(h, w, False), bands(h, w, 2),
            blocks(h, w, 2, 4), bands(h, w, 5), bands(h, w, 6), blocks(h, w, 8, 8)]


def images(segs, config_id=4):
    from gcn_grabcut.synthetic import synthetic_batch
    h, w = segs[0].shape
    return synthetic_batch(len(segs), h, w, config_id=config_id)


def run(ctx, segs, bgr, conn, k, lab_edit=None):
    """-> (graph dict, host arrays seg, lab, hsv, grad) of one ggc_graph_count / ggc_graph_fill on the label maps."""
    import torch
    import gpu_helpers as gh
    _, lab, hsv, gray, grad = gh.preprocess(ctx, bgr)
    if lab_edit is not None:
        lab = torch.as_tensor(lab_edit(lab.cpu().numpy())).cuda()
    seg = np.stack(segs).astype(np.int32)
    nn = np.array([int(s.max()) + 1 for s in segs], np.int32)
    g = gh.graph(ctx, torch.as_tensor(seg).cuda(), torch.as_tensor(nn).cuda(), lab, hsv, grad, conn, k)
    torch.cuda.synchronize()
    return g, seg, lab.cpu().numpy(), hsv.cpu().numpy(), grad.cpu().numpy()


def digest(g):
    """One hash over every output of a graph build, byte for byte."""
    m = hashlib.sha256()
    m.update(g["node_ptr"].tobytes())
    m.update(g["edge_ptr"].tobytes())
    e = int(g["edge_ptr"][-1])
    for name in ("x", "centroids", "area"):
        m.update(g[name].cpu().numpy().tobytes())
    for name in ("src", "dst", "attr"):
        m.update(g[name][:e].cpu().numpy().tobytes())
    return m.hexdigest()
