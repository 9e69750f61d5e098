"""Float64 numpy restatement of the full-resolution closed-form matte (test infrastructure): the lift of a working-size
trimap and alpha to a larger size (ggc_lift_trimap) and the warm stop rule (ggc_trimap_matte_warm), over
tests/trimap_matte_ref.py, closed_form_ref.py and upsample_ref.py.

    lift    per output pixel (y, x) of (H1, W1): (y0, y1, wy), (x0, x1, wx) = upsample_ref.source_coords (the half-pixel
            formula of ggc_upsample_matte).  trimap_full = 255 if every source pixel of nonzero weight is 255, 0 if
            every one is 0, else 128 (x1 counts when wx > 0, y1 when wy > 0); the 128 set is then dilated by `grow`
            (Chebyshev, clipped).  alpha0_full = float32(lerp(lerp(a00, a01, wx), lerp(a10, a11, wx), wy)) with
            a = clip(alpha, 0, 1), a NaN read as 0, lerp(u, v, t) = u + t (v - u)
    warm    trimap_matte_ref.pcg's recurrence statement for statement; the residual is divided by ||r_ref||,
            r_ref = -(L x^1/2)_U with x^1/2 the known values off U and 0.5 on U, instead of by ||r_0||, and the stop test
            is made on r_0 too.  r_ref = 0 is the trivial case in r_0 = 0's place

full_scene and the chains below are what tools/full_matte_study.py and the tests run."""
from __future__ import annotations

import numpy as np

import trimap_matte_ref as tm
from closed_form_ref import Laplacian, pcg as band_pcg, strand_scene
from upsample_ref import _coord, _lerp, source_coords


def _unit(alpha) -> np.ndarray:
    a = np.asarray(alpha, np.float64)
    return np.clip(np.where(np.isnan(a), 0.0, a), 0.0, 1.0)


def lift(trimap: np.ndarray, alpha: np.ndarray, full_shape, grow: int = 0):
    """-> (trimap_full (H1, W1) uint8, alpha0_full (H1, W1) float32)."""
    t = np.asarray(trimap)
    h, w = t.shape
    h1, w1 = full_shape
    y0, y1, wy = source_coords(h1, h)
    x0, x1, wx = source_coords(w1, w)
    yb, xb = np.where(wy > 0.0, y1, y0), np.where(wx > 0.0, x1, x0)
    corners = [t[y0][:, x0], t[y0][:, xb], t[yb][:, x0], t[yb][:, xb]]
    fg = np.logical_and.reduce([c == 255 for c in corners])
    bg = np.logical_and.reduce([c == 0 for c in corners])
    out = np.where(fg, 255, np.where(bg, 0, 128)).astype(np.uint8)
    if grow > 0:
        out[tm._dilate(out == 128, grow)] = 128
    a = _unit(alpha)
    top = _lerp(a[y0][:, x0], a[y0][:, x1], wx[None, :])
    bot = _lerp(a[y1][:, x0], a[y1][:, x1], wx[None, :])
    return out, _lerp(top, bot, wy[:, None]).astype(np.float32)


def brute_force_lift(trimap: np.ndarray, alpha: np.ndarray, full_shape, grow: int = 0):
    """The same as a loop over output pixels in Python floats, the dilation as a loop over the window."""
    t = np.asarray(trimap)
    a = np.asarray(alpha, np.float64)
    h, w = t.shape
    h1, w1 = full_shape
    clamp = lambda v: 0.0 if not v >= 0.0 else (1.0 if v > 1.0 else float(v))  # noqa: E731
    base = np.zeros((h1, w1), np.uint8)
    start = np.zeros((h1, w1), np.float32)
    for y in range(h1):
        ya, yb, wy = _coord(y, h1, h)
        for x in range(w1):
            xa, xb, wx = _coord(x, w1, w)
            src = {(ya, xa)}
            if wx > 0.0:
                src.add((ya, xb))
            if wy > 0.0:
                src.add((yb, xa))
            if wx > 0.0 and wy > 0.0:
                src.add((yb, xb))
            vals = [int(t[p]) for p in src]
            base[y, x] = 255 if all(v == 255 for v in vals) else (0 if all(v == 0 for v in vals) else 128)
            start[y, x] = np.float32(_lerp(_lerp(clamp(a[ya, xa]), clamp(a[ya, xb]), wx),
                                           _lerp(clamp(a[yb, xa]), clamp(a[yb, xb]), wx), wy))
    out = base.copy()
    for y in range(h1):
        for x in range(w1):
            if (base[max(0, y - grow):y + grow + 1, max(0, x - grow):x + grow + 1] == 128).any():
                out[y, x] = 128
    return out, start


def half_image(trimap: np.ndarray) -> np.ndarray:
    """x^1/2: 1 on F, 0 on G, 0.5 on U."""
    return tm.start_image(trimap, None)


def pcg_warm(bgr: np.ndarray, trimap: np.ndarray, r: int, eps: float, max_iter: int, tol: float, alpha0):
    """-> (alpha (H, W) float64 unclamped, iterations, ||r_j|| / ||r_ref||)."""
    _, _, U = tm.regions(trimap)
    x = tm.start_image(trimap, alpha0)
    if not U.any() or U.all():
        return x, 0, 0.0
    L = Laplacian(bgr, r, eps)
    dg = L.diagonal()[U]

    def op(v):
        p = np.zeros_like(x)
        p[U] = v
        return L.apply(p)[U]

    ref = -L.apply(half_image(trimap))[U]
    r_ref = np.sqrt(ref @ ref)
    if r_ref == 0.0:
        return x, 0, 0.0
    res = -L.apply(x)[U]
    it, rel = 0, np.sqrt(res @ res) / r_ref
    if rel <= tol:
        return x, 0, rel
    z = res / dg
    d = z.copy()
    rz = res @ z
    xu = x[U].copy()
    while it < max_iter:
        q = op(d)
        a = rz / (d @ q)
        xu += a * d
        res -= a * q
        it += 1
        rel = np.sqrt(res @ res) / r_ref
        if rel <= tol:
            break
        z = res / dg
        rz_new = res @ z
        d = z + (rz_new / rz) * d
        rz = rz_new
    x[U] = xu
    return x, it, rel


def residual_norms(bgr, trimap, alpha_raw, r: int, eps: float):
    """(||(L alpha)_U||, ||(L x^1/2)_U||) in float64: what the warm entry's rel_residual is the ratio of."""
    _, _, U = tm.regions(trimap)
    L = Laplacian(bgr, r, eps)
    return (float(np.linalg.norm(L.apply(np.asarray(alpha_raw, np.float64))[U])),
            float(np.linalg.norm(L.apply(half_image(trimap))[U])))


def box_down(a: np.ndarray, k: int) -> np.ndarray:
    """(H, W[, C]) -> (H / k, W / k[, C]) float64 means of the k x k boxes (H, W multiples of k)."""
    a = np.asarray(a, np.float64)
    h, w = a.shape[0] // k, a.shape[1] // k
    return a.reshape(h, k, w, k, *a.shape[2:]).mean(axis=(1, 3))


def full_scene(h1: int = 480, w1: int = 640, k: int = 4, seed: int = 0):
    """A strand scene at (h1, w1) and its working-size version by a k x k box-down: -> (full bgr u8, true alpha f64
    (h1, w1), working bgr u8, working mask u8 = box-down of the true alpha >= 0.5)."""
    full, alpha_true, _ = strand_scene(h1, w1, radius=h1 / 3.0, seed=seed)
    work = np.rint(box_down(full, k)).astype(np.uint8)
    mask = (box_down(alpha_true, k) >= 0.5).astype(np.uint8)
    return full, alpha_true, work, mask


CF = (1, 1e-5, 1, 500, 1e-4)           # radius, eps, band, max_iter, tol: the working-size defaults
FULL_MAX_ITER = 2000


def chain(full, work, mask, grow: int = 0, tol: float = CF[4], full_max_iter: int = FULL_MAX_ITER, warm: bool = True):
    """closed_form_matte_full restated: -> dict(work_alpha, trimap_full, alpha0_full, alpha (unclamped), iters, rel)."""
    r, eps, band, max_iter, _ = CF
    wa, _, _ = band_pcg(work, mask, r, eps, band, max_iter, CF[4])
    t_full, a0 = lift(tm.trimap_from_mask(mask, band), wa, full.shape[:2], grow)
    if warm:
        a, it, rel = pcg_warm(full, t_full, r, eps, full_max_iter, tol, a0)
    else:
        a, it, rel = tm.pcg(full, t_full, r, eps, full_max_iter, tol)
    return dict(work_alpha=wa, trimap_full=t_full, alpha0_full=a0, alpha=a, iters=it, rel=rel)


def sad(alpha, alpha_true) -> float:
    """Whole-image SAD of the clamped alpha."""
    return float(np.abs(np.clip(np.asarray(alpha, np.float64), 0.0, 1.0) - alpha_true).sum())


# the scenes the device's warm solve is held to the restatement on: (h1, w1, k, seed, grow)
WARM_CASES = ((120, 160, 2, 0, 0), (120, 160, 2, 1, 0), (120, 160, 4, 0, 2), (90, 120, 3, 2, 1))


def warm_case(h1, w1, k, seed, grow):
    """-> (full bgr, lifted trimap u8, lifted start f32) of one of WARM_CASES."""
    full, _, work, mask = full_scene(h1, w1, k, seed)
    r, eps, band, max_iter, tol = CF
    wa, _, _ = band_pcg(work, mask, r, eps, band, max_iter, tol)
    t_full, a0 = lift(tm.trimap_from_mask(mask, band), wa, (h1, w1), grow)
    return full, t_full, a0
