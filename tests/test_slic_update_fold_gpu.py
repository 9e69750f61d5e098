"""k_slic_update's member lists (compact, then fold): centres, raw labels and segments bit for bit against the CPU oracle
where the lists are folded many times per cluster, never filled, filled to exactly their capacity, and on clipped windows.

The device skips the update after the tenth assignment, so its centre scratch holds the ninth update's centres and its
raw labels are the tenth assignment's.  Every case asserts its property on the oracle's output before it looks at the
device.  No case enters the kernel's `stale[b]` branch: a CPU search found no pixel outside every search window at any
of these shapes."""
import numpy as np
import pytest

import gpu_helpers as gh

pytestmark = pytest.mark.gpu

UPD_CAP = 32        # entries of a group's member list, csrc/ggc_slic.hip


def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _halves():
    img = np.empty((48, 64, 3), np.int32)
    img[:, :32] = (40, 90, 200)
    img[:, 32:] = (210, 160, 30)
    img += np.random.default_rng(0).integers(-8, 9, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def _reference(oracle, lab, n_seg, sigma, compactness=10.0):
    """-> K, member counts (9, K) of the nine updates, centres of the ninth update, raw labels, segments, n."""
    h, w = lab.shape[:2]
    x = oracle.slic_rescale_lab(lab, True)
    if sigma > 0:
        x = oracle.gaussian(x, sigma)
    x = x * np.float32(1.0 / compactness)
    g = oracle.slic_grid(h, w, n_seg)
    ys = g["start_y"] + g["step_y"] * np.arange(g["ny"])
    xs = g["start_x"] + g["step_x"] * np.arange(g["nx"])
    seeds = np.stack(np.meshgrid(ys, xs, indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
    step = float(max(g["step_y"], g["step_x"]))
    counts = np.stack([np.bincount(oracle.slic_kmeans(x, seeds, step, max_iter=it)[0].ravel(), minlength=g["K"])
                       for it in range(1, 10)])
    centers = oracle.slic_kmeans(x, seeds, step, max_iter=9)[1]
    raw = oracle.slic_kmeans(x, seeds, step, max_iter=10)[0]
    seg, n = oracle.slic(lab, n_seg, compactness, sigma, True)
    return g["K"], counts, centers, raw, seg, n


def _device(gpu_ctx, lab, n_seg, sigma, k):
    """ggc_slic on a (B, H, W, 3) device batch -> centres (B, K, 5) as uint32, raw labels, segments, n."""
    b, h, w, _ = lab.shape
    seg, n = gh.slic(gpu_ctx, lab, n_seg, 10.0, sigma)
    seg, n = seg.cpu().numpy(), n.cpu().numpy()
    centers = np.empty((b, k, 5), np.float32)
    raw = np.empty((b, h, w), np.int32)
    gpu_ctx.call("ggc_debug_read_scratch", b"slic_centers", centers.ctypes.data, centers.nbytes)
    gpu_ctx.call("ggc_debug_read_scratch", b"slic_raw_labels", raw.ctypes.data, raw.nbytes)
    return centers.view(np.uint32), raw, seg, n


def _check(oracle, gpu_ctx, bgr, n_seg, sigma, prop):
    """bgr: (B, H, W, 3) uint8.  prop(K, counts, centres) asserts the case's property on the oracle, image by image."""
    lab = gh.preprocess(gpu_ctx, bgr)[1]
    lab_h = lab.cpu().numpy()
    refs = [_reference(oracle, lab_h[i], n_seg, sigma) for i in range(len(bgr))]
    for k, counts, centers, _, _, _ in refs:
        prop(k, counts, centers)
    got_c, got_raw, got_seg, got_n = _device(gpu_ctx, lab, n_seg, sigma, refs[0][0])
    for i, (k, _, centers, raw, seg, n) in enumerate(refs):
        bad = np.flatnonzero((got_c[i] != centers.view(np.uint32)).any(axis=1))
        assert bad.size == 0, (i, bad[:8], got_c[i][bad[:2]].view(np.float32), centers[bad[:2]])
        assert np.array_equal(got_raw[i], raw), (i, int((got_raw[i] != raw).sum()))
        assert np.array_equal(got_seg[i], seg) and got_n[i] == n
    return got_c, got_raw, got_seg, got_n


@pytest.mark.parametrize("seed", range(4))
def test_clusters_far_above_the_list_capacity(oracle, gpu_ctx, seed):
    """four clusters of more than a thousand pixels: forty and more folds per cluster, half of the wave's groups idle"""
    def prop(k, counts, centers):
        assert k == 4 and 1276 <= counts.max() <= 1570 and counts.max() > 16 * UPD_CAP
    _check(oracle, gpu_ctx, _noise(seed, 64, 64)[None], 4, 1.0, prop)


def test_clusters_far_above_the_list_capacity_without_smoothing(oracle, gpu_ctx):
    def prop(k, counts, centers):
        assert k == 2 and counts.max() == 1872
    _check(oracle, gpu_ctx, _halves()[None], 2, 0.0, prop)


@pytest.mark.parametrize("seed", range(4))
def test_empty_clusters(oracle, gpu_ctx, seed):
    """a group that never appends anything ends with the 0 / 0 centre"""
    def prop(k, counts, centers):
        assert k == 256 and 1 <= int(np.isnan(centers[:, 0]).sum()) <= 2
        assert np.array_equal(np.isnan(centers[:, 0]), counts[8] == 0)
    _check(oracle, gpu_ctx, _noise(seed, 32, 32)[None], 256, 1.0, prop)


def test_odd_geometry(oracle, gpu_ctx):
    """windows clipped on all four sides; neither W nor K a multiple of 8; clusters above the capacity"""
    def prop(k, counts, centers):
        assert k == 20 and UPD_CAP < counts[8].max() <= 190 and counts.max() > 2 * UPD_CAP
    _check(oracle, gpu_ctx, _noise(0, 37, 53)[None], 20, 0.0, prop)


def test_batch_indexing(oracle, gpu_ctx):
    bgr = np.stack([_noise(10 + i, 96, 128) for i in range(3)])

    def prop(k, counts, centers):
        assert k == 154 and counts.max() > UPD_CAP
    got_c, got_raw, got_seg, got_n = _check(oracle, gpu_ctx, bgr, 150, 1.0, prop)
    assert not np.array_equal(got_raw[0], got_raw[1]) and not np.array_equal(got_raw[1], got_raw[2])
    for i in range(3):                      # each image alone
        lab = gh.preprocess(gpu_ctx, bgr[i:i + 1])[1]
        one_c, one_raw, one_seg, one_n = _device(gpu_ctx, lab, 150, 1.0, 154)
        assert np.array_equal(one_c[0], got_c[i]) and np.array_equal(one_raw[0], got_raw[i])
        assert np.array_equal(one_seg[0], got_seg[i]) and one_n[0] == got_n[i]


@pytest.mark.parametrize("seed", range(2))
def test_capacity_boundary(oracle, gpu_ctx, seed):
    """some cluster with exactly as many members as a list holds, some with twice as many and some with one fewer, in one
    of the nine updates (shape and seeds found by scanning on the CPU): the fold before a chunk is appended, off by one"""
    def prop(k, counts, centers):
        assert k == 64 and (counts == UPD_CAP).any() and (counts == 2 * UPD_CAP).any() and (counts == UPD_CAP - 1).any()
    _check(oracle, gpu_ctx, _noise(seed, 48, 48)[None], 72, 1.0, prop)
