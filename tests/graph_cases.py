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


def pair_keys(seg, conn, y0=0, y1=None):
    """Sorted keys lo * n + hi (n = seg.max() + 1) of the distinct adjacent label pairs whose first pixel lies in the rows
    [y0, y1): the links right and down, and both diagonals at connectivity 8, as k_adj takes them."""
    h, w = seg.shape
    y1 = h if y1 is None else min(y1, h)
    a = seg[y0:y1].astype(np.int64)
    below = seg[y0 + 1:y1 + 1].astype(np.int64)                    # one row shorter than a where the band ends the image
    m = below.shape[0]
    links = [(a[:, :-1], a[:, 1:]), (a[:m], below)]
    if conn == 8:
        links += [(a[:m, :-1], below[:, 1:]), (a[:m, 1:], below[:, :-1])]
    n = int(seg.max()) + 1
    keys = [np.minimum(u, v)[u != v] * n + np.maximum(u, v)[u != v] for u, v in links]
    return np.unique(np.concatenate([k.ravel() for k in keys]))


def pair_count(seg, conn):
    return len(pair_keys(seg, conn))


def band_pair_counts(seg, conn, bands):
    """Distinct pairs that each of k_region_scan's row bands meets, its links into the next band's first row included."""
    h = seg.shape[0]
    bands = min(bands, h)
    rows_per = (h + bands - 1) // bands
    return [len(pair_keys(seg, conn, min(g * rows_per, h), min((g + 1) * rows_per, h))) for g in range(bands)]


PAIR_LIMIT, NODE_LIMIT, K_LIMIT = 6144, 704, 8         # OC_PAIRS, OC_NMAX, OC_KMAX of ggc_graph.hip


def predict(segs, conn, k):
    """Which kernels one ggc_graph_count takes where the tables are tried at any batch size (GGC_GRAPH_ONCHIP=2):
    'dense' when the host gate refuses (N or k over the limit), 'overflow' when the scan runs and an image's distinct pairs
    exceed the table, so that the dense kernels follow, else 'onchip'."""
    if max(int(s.max()) + 1 for s in segs) > NODE_LIMIT or k > K_LIMIT:
        return "dense"
    return "overflow" if any(pair_count(s, conn) > PAIR_LIMIT for s in segs) else "onchip"


def relabelled(seg):
    """The same partition with the labels 0..N-1, every one present, in ascending order of the old labels."""
    return np.unique(seg, return_inverse=True)[1].reshape(seg.shape).astype(np.int32)


def euler_circuit(n):
    """Vertices of a closed walk through every edge of the complete graph K_n once (n odd), by Hierholzer."""
    assert n % 2 == 1
    unused = [set(range(n)) - {v} for v in range(n)]
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if unused[v]:
            u = min(unused[v])
            unused[v].discard(u)
            unused[u].discard(v)
            stack.append(u)
        else:
            walk.append(stack.pop())
    return walk


def exact_pairs(target, h=128, w=96, n=113):
    """A map with exactly `target` distinct adjacent pairs at connectivity 4: an Eulerian circuit of K_n runs along the even
    rows (a row starts with the label the row above it ended with), so every step of the walk is a new pair; the odd rows
    and whatever the walk leaves hold a separator label, which is one more pair per label of the walk.  The walk grows one
    pixel at a time until the count is the target."""
    walk = euler_circuit(n)

    def build(steps):
        seg = np.full((h, w), n, np.int32)
        for r in range((steps + w - 2) // (w - 1)):
            piece = walk[r * (w - 1):min(r * (w - 1) + w, steps + 1)]
            seg[2 * r, :len(piece)] = piece
            seg[2 * r, len(piece):] = piece[-1]
        return seg

    steps = max(1, target - n - 1)
    while pair_count(build(steps), 4) < target:
        steps += 1
        assert steps < len(walk) and (steps + w - 2) // (w - 1) <= (h + 1) // 2, "the walk does not reach the target"
    seg = relabelled(build(steps))
    assert pair_count(seg, 4) == target
    return seg


def one_band_overflow(seed=11):
    """256 x 96 of 8 x 8 blocks whose top 32 rows are scattered labels: of eight row bands the first alone holds more pairs
    than the table, the others a few hundred.  N = 704."""
    seg = blocks(256, 96, 8, 8)
    seg[:32] = scattered(32, 96, NODE_LIMIT, seed)
    return seg


def voronoi(h, w, n, seed):
    """Nearest-site labels of n random sites: planar, irregular regions with hubs and slivers.  Sites that own no pixel
    drop out, the labels are 0..N-1 with N <= n."""
    rng = np.random.default_rng(seed)
    sy, sx = rng.integers(0, h, n), rng.integers(0, w, n)
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = (yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2
    return relabelled(np.argmin(d2, axis=-1))


def region_limit(n):
    """44 x 64 of 2 x 2 blocks is 704 regions, the most the on-chip tables hold; 703 merges the last two, 705 splits a pixel
    off the last."""
    seg = blocks(44, 64, 2, 2)
    if n == NODE_LIMIT - 1:
        seg[seg == NODE_LIMIT - 1] = NODE_LIMIT - 2
    elif n == NODE_LIMIT + 1:
        seg[-1, -1] = NODE_LIMIT
    else:
        assert n == NODE_LIMIT
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


def traced(ctx, call):
    """-> (call(), path): which topology kernels the ggc_graph_count inside `call` launched, from the profiler's scopes:
    'onchip' (k_region_scan and no dense matrix), 'overflow' (the scan, then the dense kernels) or 'dense' (no scan)."""
    ctx.profile_enable(1)
    try:
        out = call()
        launches = (ctx.profile_query("graph_scan")[0], ctx.profile_query("graph_dense")[0])
    finally:
        ctx.profile_enable(0)
    return out, {(1, 0): "onchip", (1, 1): "overflow", (0, 1): "dense"}.get(launches, "scan=%d dense=%d" % launches)


def flat_lab(lab):
    """One colour everywhere, in numbers whose sums are exact: every mean-Lab distance is 0."""
    lab[...] = np.array([50.0, 10.0, -10.0], np.float32)
    return lab


# The limits of the on-chip tables (704 regions, 6144 distinct pairs, k = 8) and the row bands of the scan.
# name -> (label maps, connectivity, k_nl, edit of the Lab image or None, the path GGC_GRAPH_ONCHIP=2 must take);
# the order matters: a case after an overflow shares its context.
LIMIT_CASES = {
    # fewer rows than bands, one row, and 9 rows, which eight bands take two at a time: the last three bands are empty
    "rows3": (lambda: [stripes(3, 70, False)], 8, 4, None, "onchip"),
    "rows1": (lambda: [blocks(1, 200, 1, 8)], 8, 4, None, "onchip"),
    "rows9": (lambda: [blocks(9, 70, 2, 8), stripes(9, 70, False)], 8, 4, None, "onchip"),
    # one below, at and one above the pair table's 6144 entries (connectivity 4, where exact_pairs is exact); one band
    # overflows in the scan's insert, several bands in k_topology's union count; then a fitting batch on the same context
    "pairs6143": (lambda: [exact_pairs(6143)], 4, 4, None, "onchip"),
    "pairs6144": (lambda: [exact_pairs(6144)], 4, 4, None, "onchip"),
    "pairs6145": (lambda: [exact_pairs(6145), blocks(128, 96, 16, 16)], 4, 4, None, "overflow"),
    "after_6145": (lambda: [blocks(128, 96, 8, 8), exact_pairs(6144)], 4, 4, None, "onchip"),
    # of eight bands the first alone overflows its table, next to a small image that fits
    "one_band_overflow": (lambda: [one_band_overflow(), blocks(256, 96, 16, 16)], 8, 4, None, "overflow"),
    "after_band_overflow": (lambda: [blocks(256, 96, 16, 16)], 8, 4, None, "onchip"),
    # one below, at and one above the 704 regions: the last bitset word is full at 704, and 705 never reaches the scan
    "n703_k8": (lambda: [region_limit(703)], 8, 8, None, "onchip"),
    "n704_k8": (lambda: [region_limit(704)], 8, 8, None, "onchip"),
    "n705_k8": (lambda: [region_limit(705)], 8, 8, None, "dense"),
    "n703_k4": (lambda: [region_limit(703)], 8, 4, None, "onchip"),
    "n704_k4": (lambda: [region_limit(704)], 8, 4, None, "onchip"),
    "n705_k4": (lambda: [region_limit(705)], 8, 4, None, "dense"),
    "ragged704": (lambda: [region_limit(704), np.zeros((44, 64), np.int32), bands(44, 64, 5)], 8, 8, None, "onchip"),
    # k = 5 is the first use of the 8-wide k-NN rows; N = k + 2 is the first with non-local pairs, N = k + 1 has none
    "voronoi_k5": (lambda: [voronoi(48, 64, 60, 1)], 8, 5, None, "onchip"),
    "voronoi_k0": (lambda: [voronoi(48, 64, 60, 2)], 8, 0, None, "onchip"),
    "n10_k8": (lambda: [bands(24, 40, 10)], 4, 8, None, "onchip"),
    "n9_k8": (lambda: [bands(24, 40, 9)], 4, 8, None, "onchip"),
    # every distance is 0: the choice is the lowest j that is not adjacent and nothing else
    "flat_k4": (lambda: [voronoi(48, 64, 60, 3)], 8, 4, flat_lab, "onchip"),
    "flat_k8": (lambda: [voronoi(48, 64, 60, 4)], 8, 8, flat_lab, "onchip"),
}


# ---- the seeded fuzz: 40 batches, most of which fit the tables.  The seed is chosen so that of the cases i = c, c + 3, ...
# (c = 0, 1, 2: one child process each) at least 10 stay on chip and at least one overflows, and one batch in all has too
# many regions for the scan; test_graph_cases_cpu.py holds it to that.
FUZZ_SEED, FUZZ_COUNT, FUZZ_PARTS = 5, 40, 3
FUZZ_KINDS = ("voronoi", "slic", "scattered", "blocks")


def fuzz_case(i, seed=FUZZ_SEED):
    """Parameters of fuzz case i: H and W in 1..130 (case 0 is one row, case 1 one column), 1 to 6 images of ragged N,
    connectivity 4 or 8, k in 0..8, and per image what its kind of map needs."""
    rng = np.random.default_rng([seed, i])
    h, w = (int(v) for v in rng.integers(1, 131, 2))
    if i == 0: h = 1
    if i == 1: w = 1
    kind = FUZZ_KINDS[int(rng.integers(0, 4))] if i >= 4 else FUZZ_KINDS[i]
    if kind == "slic" and min(h, w) < 16:
        kind = "voronoi"                                  # SLIC wants room for its seed grid
    b, conn, k = int(rng.integers(1, 7)), int(rng.choice([4, 8])), int(rng.integers(0, 9))
    case = dict(i=i, seed=seed, h=h, w=w, kind=kind, b=b, conn=conn, k=k, config_id=int(rng.integers(0, 9)))
    if kind == "voronoi":
        case["n"] = [int(v) for v in rng.integers(1, min(h * w, 160) + 1, b)]
    elif kind == "slic":
        case["n_seg"] = int(rng.integers(8, 150))
    elif kind == "scattered":
        # room for more than 6144 pairs; up to 105 labels have at most 5460, one image of 180 or more goes well over
        case["h"], case["w"] = (int(v) for v in rng.integers(70, 131, 2))
        case["n"] = [int(v) for v in rng.integers(40, 106, b)]
        if rng.random() < 0.4:
            case["n"][int(rng.integers(0, b))] = int(rng.integers(180, 400))
    else:
        case["block"] = [tuple(int(v) for v in rng.integers(2, 17, 2)) for _ in range(b)]       # at most 65 x 65 blocks
    case["map_seed"] = [int(v) for v in rng.integers(0, 1 << 30, b)]
    return case


def fuzz_maps(case, slic):
    """The label maps of one fuzz case; slic(bgr [b, h, w, 3], n_seg) -> list of label maps (the device's, or the oracle's
    where no device is at hand)."""
    h, w, b = case["h"], case["w"], case["b"]
    if case["kind"] == "voronoi":
        return [voronoi(h, w, n, s) for n, s in zip(case["n"], case["map_seed"])]
    if case["kind"] == "scattered":
        return [scattered(h, w, min(n, h * w), s) for n, s in zip(case["n"], case["map_seed"])]
    if case["kind"] == "blocks":
        return [blocks(h, w, bh, bw) for bh, bw in case["block"]]
    from gcn_grabcut.synthetic import synthetic_batch
    return slic(synthetic_batch(b, h, w, config_id=case["config_id"]), case["n_seg"])
