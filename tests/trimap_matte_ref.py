"""Float64 numpy restatement of the trimap matte (test infrastructure): the closed-form matte of tests/closed_form_ref.py
with the unknown set, the known values and the start taken from a trimap instead of from a mask's edge.

    F = {trimap == 255}, G = {trimap == 0}, U = every other byte; alpha = 1 on F, 0 on G
    start: alpha_U = clip(alpha0, 0, 1), or 0.5 without alpha0
    L_UU alpha_U = -L_{U,F} 1_F by Jacobi-preconditioned CG, stopped on ||r_j|| <= tol ||r_0|| or at max_iter, with
    r_0 = -(L x0)_U from ONE application of L to the whole start image x0 (known values off U, the start on U)
    U empty, U everything (singular: nothing anchors it) or r_0 = 0: the start, 0 iterations, relative residual 0

The recurrence is closed_form_ref.pcg's statement for statement, so that with trimap_from_mask(mask, band) and
alpha0 = mask the two return the same floats."""
from __future__ import annotations

import numpy as np

from closed_form_ref import Laplacian, dense_laplacian, unknown_band


def regions(trimap: np.ndarray):
    """-> (F, G, U) boolean maps."""
    t = np.asarray(trimap)
    F, G = t == 255, t == 0
    return F, G, ~(F | G)


def start_image(trimap: np.ndarray, alpha0=None) -> np.ndarray:
    """x0 (H, W) float64: 1 on F, 0 on G, the clamped start on U."""
    F, _, U = regions(trimap)
    x = F.astype(np.float64)
    x[U] = 0.5 if alpha0 is None else np.clip(np.asarray(alpha0, np.float64), 0.0, 1.0)[U]
    return x


def pcg(bgr: np.ndarray, trimap: np.ndarray, r: int, eps: float, max_iter: int, tol: float, alpha0=None):
    """-> (alpha (H, W) float64 unclamped, iterations, ||r_j|| / ||r_0||)."""
    _, _, U = regions(trimap)
    x = start_image(trimap, alpha0)
    if not U.any() or U.all():
        return x, 0, 0.0
    L = Laplacian(bgr, r, eps)
    dg = L.diagonal()[U]

    def op(v):
        p = np.zeros_like(x)
        p[U] = v
        return L.apply(p)[U]

    res = -L.apply(x)[U]
    r0 = np.sqrt(res @ res)
    if r0 == 0.0:
        return x, 0, 0.0
    z = res / dg
    d = z.copy()
    rz = res @ z
    xu = x[U].copy()
    it, rel = 0, 1.0
    while it < max_iter:
        q = op(d)
        a = rz / (d @ q)
        xu += a * d
        res -= a * q
        it += 1
        rel = np.sqrt(res @ res) / r0
        if rel <= tol:
            break
        z = res / dg
        rz_new = res @ z
        d = z + (rz_new / rz) * d
        rz = rz_new
    x[U] = xu
    return x, it, rel


def direct_solve(bgr: np.ndarray, trimap: np.ndarray, r: int, eps: float, alpha0=None) -> np.ndarray:
    """The same system by numpy.linalg.solve on the dense L (tiny images only); the start where the system is trivial."""
    _, _, U = regions(trimap)
    x = start_image(trimap, alpha0).reshape(-1)
    u = U.reshape(-1)
    if u.any() and not u.all():
        L = dense_laplacian(bgr, r, eps)
        x[u] = np.linalg.solve(L[np.ix_(u, u)], -L[np.ix_(u, ~u)] @ x[~u])
    return x.reshape(U.shape)


def residual_norms(bgr, trimap, alpha_raw, r: int, eps: float, alpha0=None):
    """(||(L alpha)_U||, ||(L x0)_U||) in float64, the certificate the device's rel_residual is checked against."""
    _, _, U = regions(trimap)
    L = Laplacian(bgr, r, eps)
    return (float(np.linalg.norm(L.apply(np.asarray(alpha_raw, np.float64))[U])),
            float(np.linalg.norm(L.apply(start_image(trimap, alpha0))[U])))


def _dilate(m: np.ndarray, k: int) -> np.ndarray:
    """Chebyshev dilation of a boolean map by k, clipped to the image."""
    h, w = m.shape
    p = np.zeros((h + 2 * k, w + 2 * k), bool)
    p[k:k + h, k:k + w] = m
    out = np.zeros_like(m, dtype=bool)
    for dy in range(2 * k + 1):
        for dx in range(2 * k + 1):
            out |= p[dy:dy + h, dx:dx + w]
    return out


def trimap_from_alpha(alpha_true: np.ndarray, k: int) -> np.ndarray:
    """128 on the Chebyshev dilation by k of {0 < alpha* < 1}, else 255 (alpha* >= 0.5)."""
    a = np.asarray(alpha_true, np.float64)
    t = np.where(a >= 0.5, 255, 0).astype(np.uint8)
    t[_dilate((a > 0.0) & (a < 1.0), k)] = 128
    return t


def trimap_from_mask(mask: np.ndarray, band: int) -> np.ndarray:
    """128 on closed_form_ref.unknown_band(mask, band), else 255 mask."""
    m = np.asarray(mask) != 0
    t = np.where(m, 255, 0).astype(np.uint8)
    t[unknown_band(mask, band)] = 128
    return t


def region_sad(alpha, alpha_true, region) -> float:
    return float(np.abs(np.asarray(alpha, np.float64) - alpha_true)[region].sum())
