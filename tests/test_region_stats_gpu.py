"""Region statistics (k_stats) on hand-made label maps whose sums are sensitive to the order of the additions.

The region sums are float64 running sums in raster order (np.bincount(weights=...)).  With ordinary images a float64 sum
of float32 values is almost always exact, so a kernel that added in another order would still pass.  Here a third of
every region's pixels are +1e17 and another third -1e17 (they cancel exactly), the rest is O(1)-O(100) noise: what
survives of the noise depends on when the running sum sits at +-1e17.  Every case first asserts in numpy that reversing
the order of the additions changes the float32 value of the Lab channel-1 sum in at least 80 % of the regions of six or
more pixels, so a change to the generator cannot quietly blunt the test.

The label maps are the smallest at which a kernel that gives a group of lanes to a region can go wrong: nested boxes,
boxes that are the whole image with members alternating inside every chunk, one region per pixel, fewer regions than
a wave holds, region counts that are no multiple of the regions per wave, and a ragged batch."""
import numpy as np
import pytest
import torch

import gpu_helpers as gh

pytestmark = pytest.mark.gpu


def _rings(h, w, t):
    yy, xx = np.mgrid[0:h, 0:w]
    return (np.minimum(np.minimum(yy, h - 1 - yy), np.minimum(xx, w - 1 - xx)) // t).astype(np.int32)


def _combs(h, w):
    """Two sets of one-pixel teeth that swap columns half-way down: both boxes are the whole image."""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx + (yy >= h // 2)) % 2).astype(np.int32)


def _pixels(h, w):
    return np.arange(h * w, dtype=np.int32).reshape(h, w)


def _giant(h, w):
    seg = np.zeros((h, w), np.int32)
    seg[5, 7], seg[h // 2 + 2, w // 2 + 4], seg[h - 1, w - 1] = 1, 2, 3
    return seg


def _single(h, w):
    return np.zeros((h, w), np.int32)


def _blocks(h, w, s):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy // s) * ((w + s - 1) // s) + xx // s).astype(np.int32)


CASES = {
    "rings3": (lambda: _rings(37, 53, 3), 7),
    "rings1": (lambda: _rings(33, 65, 1), 17),
    "combs": (lambda: _combs(40, 63), 2),
    "pixels": (lambda: _pixels(12, 12), 144),
    "giant": (lambda: _giant(37, 53), 4),
    "single": (lambda: _single(24, 17), 1),
    "blocks5": (lambda: _blocks(41, 67, 5), 126),
    "blocks7": (lambda: _blocks(96, 130, 7), 266),
}


def _seg(name):
    make, n = CASES[name]
    seg = make()
    assert np.array_equal(np.unique(seg), np.arange(n)), name      # all labels 0..N-1 are present
    return seg, n


def _cancelling_plane(seg, rng, absolute=False):
    """Per region: a third +1e17, a third -1e17 (seeded permutation), the rest noise."""
    out = np.empty(seg.shape, np.float32)
    flat, lab = out.reshape(-1), seg.reshape(-1)
    for r in range(int(seg.max()) + 1):
        idx = np.flatnonzero(lab == r)
        v = rng.uniform(-100.0, 100.0, idx.size).astype(np.float32)
        third = idx.size // 3
        perm = rng.permutation(idx.size)
        v[perm[:third]] = 1e17
        v[perm[third:2 * third]] = -1e17
        flat[idx] = v
    return np.abs(out) if absolute else out


def _adversarial_inputs(seg, seed):
    rng = np.random.default_rng(seed)
    lab = np.stack([_cancelling_plane(seg, rng) for _ in range(3)], axis=-1)
    hsv = np.stack([_cancelling_plane(seg, rng) for _ in range(3)], axis=-1)
    grad = _cancelling_plane(seg, rng, absolute=True)
    return np.ascontiguousarray(lab), np.ascontiguousarray(hsv), grad


def _order_sensitive_share(seg, plane):
    """Share of the regions of >= 6 pixels whose float32 sum changes when the additions run backwards."""
    flat, lab = plane.reshape(-1).astype(np.float64), seg.reshape(-1)
    n_big = n_sens = 0
    for r in range(int(seg.max()) + 1):
        v = flat[lab == r]                                          # raster order
        if v.size < 6:
            continue
        n_big += 1
        fwd, bwd = np.cumsum(v)[-1], np.cumsum(v[::-1])[-1]         # cumsum is the plain running sum
        n_sens += np.float32(fwd) != np.float32(bwd)
    return n_big, n_sens


def _check_image(oracle, g, i, seg_h, lab_h, hsv_h, grad_h, conn, k, want=None):
    if want is None:
        want = oracle.graph_build(seg_h, lab_h, hsv_h, grad_h, connectivity=conn, n_nonlocal=k)
    n0, n1 = g["node_ptr"][i], g["node_ptr"][i + 1]
    e0, e1 = g["edge_ptr"][i], g["edge_ptr"][i + 1]
    assert n1 - n0 == want["n_nodes"] and e1 - e0 == want["n_edges"]
    x = g["x"][n0:n1].cpu().numpy()
    assert np.array_equal(x[:, :16], want["node_features"])
    assert np.array_equal(x[:, 16:], want["prior"])
    assert np.array_equal(g["centroids"][n0:n1].cpu().numpy(), want["centroids"])
    assert np.array_equal(g["area"][n0:n1].cpu().numpy(), want["area_ratio"])
    ei = np.stack([g["src"][e0:e1].cpu().numpy(), g["dst"][e0:e1].cpu().numpy()]).astype(np.int64)
    assert np.array_equal(ei, want["edge_index"])
    if e1 > e0:
        assert np.array_equal(g["attr"][e0:e1].cpu().numpy(), want["edge_attr"])
    return want


def _assert_finite(want):
    for key in ("node_features", "prior", "edge_attr"):
        assert np.isfinite(want[key]).all(), key


def _run(gpu_ctx, segs, nns, lab, hsv, grad, conn, k=4):
    seg_d = torch.as_tensor(np.stack(segs)).cuda()
    nn_d = torch.as_tensor(np.array(nns, np.int32)).cuda()
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    return gh.graph(gpu_ctx, seg_d, nn_d, to(lab), to(hsv), to(grad), conn, k)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", list(CASES))
def test_region_stats_order_sensitive_inputs(oracle, gpu_ctx, name, conn):
    seg, n = _seg(name)
    lab, hsv, grad = _adversarial_inputs(seg, seed=sorted(CASES).index(name))
    n_big, n_sens = _order_sensitive_share(seg, lab[..., 1])
    if name != "pixels":                                            # no region of >= 6 pixels there
        assert n_big > 0 and n_sens >= 0.8 * n_big, (name, n_big, n_sens)
    want = oracle.graph_build(seg, lab, hsv, grad, connectivity=conn, n_nonlocal=4)
    _assert_finite(want)
    g = _run(gpu_ctx, [seg], [n], lab[None], hsv[None], grad[None], conn)
    _check_image(oracle, g, 0, seg, lab, hsv, grad, conn, 4, want)


def test_region_stats_ragged_batch(oracle, gpu_ctx):
    h, w = 37, 53
    segs = [_rings(h, w, 3), _giant(h, w), _blocks(h, w, 5)]
    nns = [7, 4, 88]
    for s, n in zip(segs, nns):
        assert np.array_equal(np.unique(s), np.arange(n))
    ins = [_adversarial_inputs(s, seed=100 + i) for i, s in enumerate(segs)]
    lab, hsv, grad = (np.stack([t[j] for t in ins]) for j in range(3))
    for conn in (4, 8):
        g = _run(gpu_ctx, segs, nns, lab, hsv, grad, conn)
        assert list(np.diff(g["node_ptr"])) == nns
        for i in range(3):
            _assert_finite(_check_image(oracle, g, i, segs[i], lab[i], hsv[i], grad[i], conn, 4))


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", list(CASES))
def test_region_stats_ordinary_inputs(oracle, gpu_ctx, name, conn):
    from gcn_grabcut.synthetic import synthetic_batch
    seg, n = _seg(name)
    h, w = seg.shape
    _, lab, hsv, _, grad = gh.preprocess(gpu_ctx, synthetic_batch(1, h, w, config_id=6))
    g = gh.graph(gpu_ctx, torch.as_tensor(seg[None]).cuda(), torch.as_tensor(np.array([n], np.int32)).cuda(), lab, hsv,
                 grad, conn, 4)
    _check_image(oracle, g, 0, seg, lab[0].cpu().numpy(), hsv[0].cpu().numpy(), grad[0].cpu().numpy(), conn, 4)
