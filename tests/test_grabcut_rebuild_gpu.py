"""The graph rebuild of ggc_grabcut between its iterations: warm balance update (mf_warm_pixel), n-link capacities computed
by the cold build, estimateSegmentation applied inside the next iteration's component assignment.

(a) ggc_grid_maxflow over four steps: every step's cut equals the oracle's, the last state certifies and satisfies the
    balance the warm update relies on, ex - snk == tw_last + sum (rc - cap).
(b) ggc_grabcut from a trimap with n_iter = 0, 1, 2, 5: mask and models after k iterations equal the oracle's k-th
    iteration (the relabel that the next iteration applies, and the last one that has no successor), with a skipped image
    and a promoted trimap in the batch; a mode-2 call continues the chain; `binary` does not change `mask`.
(c) images of height 1 and width 1: links that leave the image carry nothing."""
import functools

import numpy as np
import pytest
import torch

import gpu_helpers as gh
import grabcut_ref as gr
import maxflow_nets as mn
from test_grabcut_gpu import _grabcut

pytestmark = pytest.mark.gpu

GRID_SHAPES = [(1, 1), (1, 257), (257, 1), (2, 33), (8, 32), (33, 65)]
N_ITERS = [0, 1, 2, 5]
SEED = 11


# ------------------------------------------------------------------------------------------------ (a)
def _grid_net(family, h, w):
    if family == "warm":
        return mn.make("warm", "resample", h, w, seed=21)
    # the four extremes share one nw (every link at 2^24): their t-links in turn are four steps with |tw| = 2^27 throughout
    # and changes of 2^28
    nets = [mn.make("extremes", v, h, w, seed=21) for v in mn.VARIANTS["extremes"]]
    assert all(np.array_equal(n, nets[0][1]) for _, n in nets)
    return np.ascontiguousarray(np.concatenate([t for t, _ in nets])), nets[0][1]


@pytest.mark.parametrize("family", ["warm", "extremes"])
@pytest.mark.parametrize("h,w", GRID_SHAPES)
def test_four_steps_match_oracle_and_keep_the_balance(gpu_ctx, oracle, family, h, w):
    tw, nw = _grid_net(family, h, w)
    assert tw.shape[0] == 4
    side, res = mn.solve(gpu_ctx, [(tw, nw)])
    for s in range(4):
        flow, want = oracle.grid_maxflow(tw[s], nw)
        assert np.array_equal(side[s, 0], want), f"{family} {h}x{w} step {s}: {int((side[s, 0] != want).sum())} pixels differ"
    mn.certify(tw[3], nw, side[3, 0], res[0], flow)
    r = res[0].astype(np.int64)
    cap = mn._arc_caps(nw)                                 # rebuilt from nw, in-image links only
    bad = r[:, :, 8] - r[:, :, 9] != tw[3].astype(np.int64) + (r[:, :, :8] - cap).sum(axis=2)
    assert not bad.any(), np.argwhere(bad)[:4].tolist()


# ------------------------------------------------------------------------------------------------ (b)
def _ramp(h, w, seed):
    """A radial colour ramp with a little noise under a trimap whose probable foreground is far too large: the GMMs and the
    cut move in every one of the first five iterations (on the synthetic scenes at this size the first cut is final)."""
    rng = np.random.default_rng([seed, h, w])
    ys, xs = np.mgrid[0:h, 0:w]
    r = np.sqrt(((ys - h / 2) / (h * 0.5)) ** 2 + ((xs - w / 2) / (w * 0.5)) ** 2)
    t = np.clip(1.3 - 1.6 * r, 0, 1)[..., None]
    c0, c1 = rng.integers(30, 100, 3), rng.integers(150, 230, 3)
    img = np.clip(c0 + (c1 - c0) * t + rng.normal(0, 4, (h, w, 3)), 0, 255).astype(np.uint8)
    tri = np.where(r < 0.8, gr.GC_PR_FGD, gr.GC_PR_BGD).astype(np.uint8)
    tri[:2] = gr.GC_BGD; tri[-2:] = gr.GC_BGD; tri[:, :2] = gr.GC_BGD; tri[:, -2:] = gr.GC_BGD
    tri[h // 2 - 1:h // 2 + 2, w // 2 - 1:w // 2 + 2] = gr.GC_FGD
    return img, tri


def _batch(h, w, n):
    pairs = [_ramp(h, w, i) for i in range(n)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


@functools.lru_cache(maxsize=None)
def _cases():
    """Two batches: three images of 33x65 (image 1 all probable background: promoted to definite, skipped; image 2 without
    definite foreground: its probable foreground is promoted) and two of 48x64."""
    imgs_a, tris_a = _batch(33, 65, 3)
    tris_a[1] = gr.GC_PR_BGD
    tris_a[2] = np.where(tris_a[2] == gr.GC_FGD, gr.GC_PR_FGD, tris_a[2])
    assert not (tris_a[2] == gr.GC_FGD).any() and (tris_a[2] == gr.GC_BGD).any()
    imgs_b, tris_b = _batch(48, 64, 2)
    return (imgs_a, tris_a), (imgs_b, tris_b)


@functools.lru_cache(maxsize=None)
def _reference(batch, i, k):
    from oracle import oracle as orc
    imgs, tris = _cases()[batch]
    return orc.grabcut(imgs[i], tris[i], n_iter=k, mode=0, seed=SEED + i)


@pytest.mark.parametrize("k", N_ITERS)
@pytest.mark.parametrize("batch", [0, 1])
def test_kth_iteration_equals_reference(gpu_ctx, oracle, batch, k):
    imgs, tris = _cases()[batch]
    binary, mask, bgd, fgd = _grabcut(gpu_ctx, imgs, tris, n_iter=k, mode=0, seed=SEED)
    for i in range(len(imgs)):
        wb, wm, wbgd, wfgd, rc = _reference(batch, i, k)
        want0, degenerate = gr.init_trimap(tris[i])
        assert rc == (1 if degenerate else 0)
        assert degenerate == (batch == 0 and i == 1)
        if degenerate:
            assert np.array_equal(mask[i], want0), (i, k)
            continue
        assert np.array_equal(mask[i], wm), (i, k, int((mask[i] != wm).sum()))
        assert np.array_equal(binary[i], wb), (i, k)
        assert np.array_equal(bgd[i], wbgd) and np.array_equal(fgd[i], wfgd), (i, k)
    if batch == 0:
        assert (mask[2][tris[2] == gr.GC_PR_FGD] == gr.GC_FGD).all()              # the promotion held through the iterations
    if k > 0:                                # the case itself: the reference's mask moved since the previous n_iter of the list
        prev = N_ITERS[N_ITERS.index(k) - 1]
        assert not np.array_equal(_reference(batch, 0, k)[1], _reference(batch, 0, prev)[1])


@pytest.mark.parametrize("batch", [0, 1])
def test_eval_mode_continues_the_chain(gpu_ctx, oracle, batch):
    imgs, tris = _cases()[batch]
    keep = [i for i in range(len(imgs)) if not gr.init_trimap(tris[i])[1]]
    _, m2, bgd, fgd = _grabcut(gpu_ctx, imgs, tris, n_iter=2, mode=0, seed=SEED)
    _, m3, _, _ = _grabcut(gpu_ctx, imgs[keep], m2[keep], n_iter=1, mode=2, bgd=bgd[keep], fgd=fgd[keep])
    for j, i in enumerate(keep):
        assert np.array_equal(m3[j], _reference(batch, i, 3)[1]), i


@pytest.mark.parametrize("k", [1, 2])
def test_mask_is_the_same_without_binary(gpu_ctx, k):
    imgs, tris = _cases()[1]
    b, h, w, _ = imgs.shape
    _, with_binary, bg1, fg1 = _grabcut(gpu_ctx, imgs, tris, n_iter=k, mode=0, seed=SEED)
    dimg, dmask = torch.as_tensor(imgs).cuda(), torch.as_tensor(tris).cuda()
    dbgd = torch.zeros(b, 65, dtype=torch.float64, device="cuda")
    dfgd = torch.zeros(b, 65, dtype=torch.float64, device="cuda")
    gpu_ctx.call("ggc_grabcut", gh.stream(), b, h, w, dimg.data_ptr(), dmask.data_ptr(), None, dbgd.data_ptr(), dfgd.data_ptr(),
                 k, 0, SEED, None)
    assert np.array_equal(dmask.cpu().numpy(), with_binary)
    assert np.array_equal(dbgd.cpu().numpy(), bg1) and np.array_equal(dfgd.cpu().numpy(), fg1)


# ------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("h,w", [(1, 64), (64, 1)])
def test_single_row_and_single_column(gpu_ctx, oracle, h, w):
    rng = np.random.default_rng(5)
    n = h * w
    line = np.where(np.arange(n)[:, None] < 26, rng.integers(20, 90, (n, 3)), rng.integers(140, 230, (n, 3))).astype(np.uint8)
    tri = np.full(n, gr.GC_PR_FGD, np.uint8)
    tri[:8] = gr.GC_BGD; tri[8:30] = gr.GC_PR_BGD; tri[50:54] = gr.GC_FGD
    img, tri = line.reshape(h, w, 3), tri.reshape(h, w)
    binary, mask, bgd, fgd = _grabcut(gpu_ctx, img[None], tri[None], n_iter=2, mode=0, seed=SEED)
    wb, wm, wbgd, wfgd, rc = oracle.grabcut(img, tri, n_iter=2, mode=0, seed=SEED)
    assert rc == 0
    assert np.array_equal(mask[0], wm), int((mask[0] != wm).sum())
    assert np.array_equal(binary[0], wb)
    assert np.array_equal(bgd[0], wbgd) and np.array_equal(fgd[0], wfgd)
    assert len(np.unique(wb)) == 2                         # a cut inside the line, not a trivial one
