"""The tile-list CG core (csrc/ggc_cg.h, csrc/ggc_cg_compact.h) under its three solvers, ggc_trimap_matte,
ggc_estimate_foreground and ggc_poisson_clone (source and mixed gradients), at the smallest shapes where its pieces can go wrong: one partial tile (5 x 5), a 2 x 3 tile grid with partial edge tiles
(17 x 33), and 130 x 130 with every one of its 9 x 9 = 81 tiles listed, more than one wave, so that the per-image sum takes
its second stride.  Batches hold an image with nothing to solve between two that are solved.  max_iter is far above the
poll interval and tol is met long before it, so the early-out path runs.

Checked: a batch equals its single-image calls bit for bit in every output, iters and rel included; an image with nothing
to solve returns its start with iters == 0; convergence comes before max_iter; and the results agree with the float64
restatements (tests/trimap_matte_ref.py, tests/foreground_ref.py, tests/clone_ref.py's exact sparse solve) under the
comparisons and tolerances of test_trimap_matte_gpu.py, test_foreground_gpu.py and test_clone_gpu.py.  The restatements solved to 1e-12 are left out at 130 x 130 (seconds
on the host); the residual certificates, one application of the operator, are kept there.  On the host the restatements
take, at these tolerances: matte 6 (5 x 5, r = 2), 148 and 74 (17 x 33, r = 1, 2) and 811 (130 x 130) iterations with at
most 2.1e-4 between the 1e-4 and the 1e-12 solutions; foreground 17, 32 and 32 with at most 1.5e-4 levels; clone (Omega
the inner 3 x 3 of 5 x 5, everything but the outer ring of 17 x 33 and 130 x 130, tol 1e-9) 5, 83 and 401 with source
gradients, 5, 80 and 373 with mixed ones, at most 1.5e-5 levels from the exact solve, which takes 0.3 s at 130 x 130 and
is kept there."""
import functools

import numpy as np
import pytest
import torch

import clone_ref as cr
import foreground_ref as fr
import trimap_matte_ref as tm
import test_clone_cpu as cc
from test_clone_gpu import _clone
from test_foreground_cpu import AGREE_LEVELS, DEFAULTS
from test_trimap_matte_cpu import EPS, MAX_ITER, TAU, TOL

pytestmark = pytest.mark.gpu
CG_POLL = 8
MATTE_KEYS = ("alpha", "rgba", "raw", "iters", "rel")
MATTE_SHAPES = [(5, 5, 2), (17, 33, 1), (17, 33, 2), (130, 130, 1)]            # h, w, r
FG_SHAPES = [(5, 5), (17, 33), (130, 130)]
F32 = lambda v: float(np.float32(v))                              # the entries take eps, eps_r, omega and tol as float32
assert MAX_ITER > 10 * CG_POLL and DEFAULTS["max_iter"] > 10 * CG_POLL and cc.MAX_ITER > 10 * CG_POLL


def _stream():
    from gcn_grabcut import _native
    return _native.current_stream(0)


def _image(h, w, seed):
    from gcn_grabcut.synthetic import synthetic_image
    return synthetic_image(h, w, seed)


def _matte(ctx, bgr, trimap, r, alpha0=None):
    """ggc_trimap_matte on (B,H,W,3) / (B,H,W) uint8 arrays -> dict of device tensors."""
    bgr, trimap = torch.as_tensor(np.ascontiguousarray(bgr)).cuda(), torch.as_tensor(np.ascontiguousarray(trimap)).cuda()
    a0 = None if alpha0 is None else torch.as_tensor(np.ascontiguousarray(alpha0, np.float32)).cuda()
    b, h, w, _ = bgr.shape
    out = dict(alpha=torch.empty(b, h, w, device="cuda"), rgba=torch.empty(b, h, w, 4, dtype=torch.uint8, device="cuda"),
               raw=torch.empty(b, h, w, dtype=torch.float64, device="cuda"),
               iters=torch.empty(b, dtype=torch.int32, device="cuda"), rel=torch.empty(b, dtype=torch.float64, device="cuda"))
    ctx.call("ggc_trimap_matte", _stream(), b, h, w, bgr.data_ptr(), trimap.data_ptr(), r, EPS, MAX_ITER, TOL,
             None if a0 is None else a0.data_ptr(), *[out[k].data_ptr() for k in MATTE_KEYS])
    torch.cuda.synchronize()
    return out


def _foreground(ctx, bgr, alpha):
    """ggc_estimate_foreground at the defaults on (B,H,W,3) uint8 / (B,H,W) float32 arrays -> dict of device tensors."""
    bgr = torch.as_tensor(np.ascontiguousarray(bgr)).cuda()
    alpha = torch.as_tensor(np.ascontiguousarray(alpha, np.float32)).cuda()
    b, h, w, _ = bgr.shape
    d = DEFAULTS
    out = dict(foreground=torch.empty(b, h, w, 3, dtype=torch.uint8, device="cuda"),
               rgba=torch.empty(b, h, w, 4, dtype=torch.uint8, device="cuda"),
               raw_f=torch.empty(b, h, w, 3, dtype=torch.float64, device="cuda"),
               raw_b=torch.empty(b, h, w, 3, dtype=torch.float64, device="cuda"),
               iters=torch.empty(b, dtype=torch.int32, device="cuda"), rel=torch.empty(b, dtype=torch.float64, device="cuda"))
    ctx.call("ggc_estimate_foreground", _stream(), b, h, w, bgr.data_ptr(), alpha.data_ptr(), d["eps_r"], d["omega"],
             d["max_iter"], d["tol"], *[v.data_ptr() for v in out.values()])
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _matte_case(h, w):
    """An image and a trimap that is unknown everywhere except a 255 top row and a 0 bottom row: every tile is listed."""
    t = np.full((h, w), 128, np.uint8)
    t[0], t[-1] = 255, 0
    return _image(h, w, h + w), t


@functools.lru_cache(maxsize=None)
def _fg_case(h, w):
    """An image and an alpha that is fractional everywhere except a top row of 1 and a bottom row of 0."""
    a = np.random.default_rng(h * w).uniform(0.05, 0.95, (h, w)).astype(np.float32)
    a[0], a[-1] = 1.0, 0.0
    return _image(h, w, h * w), a


@functools.lru_cache(maxsize=None)
def _clone_batch(h, w, middle):
    """Three noise sources and targets of one size at offset (0, 0).  Omega of the first and the last is everything but
    the outer ring (5 x 5: the inner 3 x 3), so that halo fetches cross tiles in both directions; the middle image is not
    solved: an empty mask, or Omega the whole target."""
    rng = np.random.default_rng(1000 + h * w)
    s, t = (rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(2))
    m = np.zeros((h, w), np.uint8)
    m[1:-1, 1:-1] = 1
    masks = np.stack([m, np.zeros_like(m) if middle == "empty" else np.ones_like(m), m])
    return np.stack([s, s[::-1], s[:, ::-1]]), masks, np.stack([t, t[::-1], t[:, ::-1]]), np.zeros((3, 2), np.int32)


@functools.lru_cache(maxsize=None)
def _clone_exact(h, w, j, mixed):
    srcs, masks, tgts, offs = _clone_batch(h, w, "empty")
    sys_ = cr.assemble(srcs[j], masks[j], tgts[j], offs[j], mixed)
    return sys_, cr.exact(sys_)


@functools.lru_cache(maxsize=None)
def _matte_exact(h, w, r):
    img, t = _matte_case(h, w)
    x, _, rel = tm.pcg(img, t, r, EPS, 50000, 1e-12)
    assert rel <= 1e-12
    return x


@functools.lru_cache(maxsize=None)
def _fg_exact(h, w):
    img, a = _fg_case(h, w)
    s = fr.snap(a)
    F, B, _, _ = fr.pcg(img, s, DEFAULTS["eps_r"], DEFAULTS["omega"], 20000, 1e-12)
    return fr.premult_levels(s, F, B)


# ---------------------------------------------------------------- one image: early out, the restatements
@pytest.mark.parametrize("h,w,r", MATTE_SHAPES)
def test_matte_converges_early_and_agrees_with_the_restatement(gpu_ctx, h, w, r):
    img, t = _matte_case(h, w)
    o = _matte(gpu_ctx, img[None], t[None], r)
    raw, iters, rel = o["raw"][0].cpu().numpy(), int(o["iters"][0]), float(o["rel"][0])
    res, res0 = tm.residual_norms(img, t, raw, r, EPS, None)
    err = float(np.abs(raw - _matte_exact(h, w, r)).max()) if h < 100 else None
    print(f"{h}x{w} r={r}: iters {iters} rel {rel:.3e} recomputed {res / res0:.3e} err {err}")
    assert 1 <= iters < MAX_ITER and rel <= TOL, (iters, rel)
    assert abs(rel - res / res0) <= 1e-6 * (res / res0), (rel, res / res0)
    F, G, _ = tm.regions(t)
    assert np.array_equal(raw[F], np.ones(F.sum())) and np.array_equal(raw[G], np.zeros(G.sum()))
    assert np.array_equal(o["alpha"][0].cpu().numpy(), np.clip(raw, 0.0, 1.0).astype(np.float32))
    assert np.array_equal(o["rgba"][0].cpu().numpy()[..., 3], np.floor(np.clip(raw, 0, 1) * 255.0 + 0.5).astype(np.uint8))
    if err is not None:
        assert err <= TAU, err


@pytest.mark.parametrize("h,w", FG_SHAPES)
def test_foreground_converges_early_and_agrees_with_the_restatement(gpu_ctx, h, w):
    img, a = _fg_case(h, w)
    d = DEFAULTS
    o = _foreground(gpu_ctx, img[None], a[None])
    raw_f, raw_b = o["raw_f"][0].cpu().numpy(), o["raw_b"][0].cpu().numpy()
    iters, rel = int(o["iters"][0]), float(o["rel"][0])
    s = fr.snap(a)
    U = (s > 0) & (s < 1)
    res, res0 = fr.residual_norms(img, s, F32(d["eps_r"]), F32(d["omega"]), raw_f, raw_b)
    gf, gb = fr.premult_levels(s, raw_f, raw_b)
    wf, wb = _fg_exact(h, w)
    df, db = np.abs(gf - wf).max(), np.abs(gb - wb).max()
    print(f"{h}x{w}: iters {iters} rel {rel:.3e} recomputed {res / res0:.3e} premultiplied F {df:.4f} B {db:.4f} levels")
    assert 1 <= iters < d["max_iter"] and rel <= d["tol"], (iters, rel)
    assert res <= 2.0 * d["tol"] * res0, res / res0
    assert abs(rel - res / res0) <= 0.1 * (res / res0), (rel, res / res0)
    fg = o["foreground"][0].cpu().numpy()
    assert np.array_equal(fg[~U], img[~U]) and np.array_equal(fg[U], fr.to_u8(raw_f)[U])
    assert np.array_equal(o["rgba"][0].cpu().numpy()[..., 3], fr.to_u8(a.astype(np.float64)))
    assert df <= AGREE_LEVELS and db <= AGREE_LEVELS, (df, db)


# ---------------------------------------------------------------- batches with an image that is not solved
def _assert_batch_equals_singles(full, single):
    for j in range(3):
        one = single(j)
        for k in full:
            assert torch.equal(one[k][0], full[k][j]), (j, k)


@pytest.mark.parametrize("middle", ["no U", "all U"])
@pytest.mark.parametrize("h,w,r", [(17, 33, 1), (130, 130, 1)])
def test_matte_batch_with_a_trivial_image_equals_its_single_calls(gpu_ctx, h, w, r, middle):
    img, t = _matte_case(h, w)
    imgs = np.stack([img, img[::-1], img[:, ::-1]])
    a0 = np.random.default_rng(3).uniform(-0.5, 1.5, (3, h, w)).astype(np.float32)
    tris = np.stack([t, np.zeros_like(t) if middle == "no U" else np.full_like(t, 77), t[::-1]])
    full = _matte(gpu_ctx, imgs, tris, r, a0)
    _assert_batch_equals_singles(full, lambda j: _matte(gpu_ctx, imgs[j:j + 1], tris[j:j + 1], r, a0[j:j + 1]))
    iters, rel, raw = full["iters"].tolist(), full["rel"].tolist(), full["raw"].cpu().numpy()
    print(f"{h}x{w} middle {middle}: iters {iters} rel {rel}")
    assert iters[1] == 0 and rel[1] == 0.0
    want = np.zeros((h, w)) if middle == "no U" else np.clip(a0[1].astype(np.float64), 0.0, 1.0)
    assert np.array_equal(raw[1], want)                          # the start comes back
    assert all(1 <= iters[j] < MAX_ITER and rel[j] <= TOL for j in (0, 2)), (iters, rel)


@pytest.mark.parametrize("h,w", [(17, 33), (130, 130)])
def test_foreground_batch_with_a_trivial_image_equals_its_single_calls(gpu_ctx, h, w):
    img, a = _fg_case(h, w)
    imgs = np.stack([img, img[::-1], img[:, ::-1]])
    alphas = np.stack([a, np.zeros_like(a), a[:, ::-1]])
    full = _foreground(gpu_ctx, imgs, alphas)
    _assert_batch_equals_singles(full, lambda j: _foreground(gpu_ctx, imgs[j:j + 1], alphas[j:j + 1]))
    iters, rel = full["iters"].tolist(), full["rel"].tolist()
    print(f"{h}x{w}: iters {iters} rel {rel}")
    assert iters[1] == 0 and rel[1] == 0.0
    assert np.array_equal(full["foreground"][1].cpu().numpy(), imgs[1])
    assert np.array_equal(full["raw_f"][1].cpu().numpy(), imgs[1] / 255.0)
    assert np.array_equal(full["raw_b"][1].cpu().numpy(), imgs[1] / 255.0)
    assert all(1 <= iters[j] < DEFAULTS["max_iter"] and rel[j] <= DEFAULTS["tol"] for j in (0, 2)), (iters, rel)


@pytest.mark.parametrize("middle", ["empty", "whole"])
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("h,w", FG_SHAPES)
def test_clone_batch_with_a_trivial_image_equals_its_single_calls_and_the_exact_solve(gpu_ctx, h, w, mixed, middle):
    srcs, masks, tgts, offs = _clone_batch(h, w, middle)
    full = _clone(gpu_ctx, srcs, masks, tgts, offs, mixed)
    _assert_batch_equals_singles(
        full, lambda j: _clone(gpu_ctx, srcs[j:j + 1], masks[j:j + 1], tgts[j:j + 1], offs[j:j + 1], mixed))
    iters, rel, n = full["iters"].tolist(), full["rel"].tolist(), full["n_omega"].tolist()
    comp, raw = full["composite"].cpu().numpy(), full["raw"].cpu().numpy()
    print(f"{h}x{w} mixed={mixed} middle {middle}: |Omega| {n} iters {iters} rel {rel}")
    assert iters[1] == 0 and rel[1] == 0.0
    want = tgts[1] if middle == "empty" else srcs[1]             # the target, or the pasted source
    assert n[1] == (0 if middle == "empty" else h * w)
    assert np.array_equal(comp[1], want) and np.array_equal(raw[1], want.astype(np.float64))
    for j in (0, 2):
        sys_, exact = _clone_exact(h, w, j, mixed)
        om = sys_["omega"]
        res, res0 = cr.residual_norms(sys_, raw[j])
        err = np.abs(raw[j][om] - exact).max()
        print(f"image {j}: residual {res / res0:.3e} |raw - exact| {err:.2e} levels")
        assert n[j] == (h - 2) * (w - 2) and 1 <= iters[j] < cc.MAX_ITER, (n, iters)
        assert res <= 2.0 * F32(cc.TOL) * res0, res / res0
        assert np.array_equal(comp[j][~om], tgts[j][~om]) and np.array_equal(comp[j][om], cr.to_bytes(raw[j][om]))
        assert err <= cc.AGREE_LEVELS, (j, err)
