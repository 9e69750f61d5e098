"""Float64 numpy restatement of the closed-form alpha matte (test infrastructure), written from Levin, Lischinski and
Weiss, "A Closed-Form Solution to Natural Image Matting" (TPAMI 2008, eq. 12: the matting Laplacian) and He, Sun and
Tang, "Fast Matting Using Large Kernel Matting Laplacian Matrices" (CVPR 2010, eqs. 9-11: L p without the matrix).

With I_i = bgr_i / 255, windows w_k of n = (2r+1)^2 pixels whose centres k lie in K = {r <= y < H-r, r <= x < W-r}:

    Delta_k = Sigma_k + (eps / n) U,   (L_k)_ij = delta_ij - (1/n) (1 + (I_i - mu_k)^T Delta_k^-1 (I_j - mu_k))
    L = sum_k L_k
    L p:  a_k = Delta_k^-1 (mean_k(I p) - mu_k mean_k(p)),  b_k = mean_k(p) - a_k . mu_k,
          (L p)_i = c_i p_i - sum_{k in K, i in w_k} (a_k . I_i + b_k),  c_i = #{k in K : i in w_k}

The unknown band U is matte_ref.edge_band(mask, band); alpha = mask off U and L_UU alpha_U = -L_{U,known} mask_known,
solved by Jacobi-preconditioned conjugate gradients from alpha = mask.  dense_laplacian assembles L window by window for
tiny images; laplacian_apply and laplacian_diagonal are the box-sum forms the device uses."""
from __future__ import annotations

import numpy as np

from matte_ref import _smooth_texture, edge_band


def _valid_box(a: np.ndarray, r: int) -> np.ndarray:
    """Sums over the (2r+1)^2 windows that lie wholly inside the image: (H, W[, ...]) -> (H-2r, W-2r[, ...])."""
    k = 2 * r + 1
    c = np.concatenate([np.zeros_like(a[:, :1]), a.cumsum(1)], axis=1)
    rows = c[:, k:] - c[:, :-k]
    c = np.concatenate([np.zeros_like(rows[:1]), rows.cumsum(0)], axis=0)
    return c[k:] - c[:-k]


def _scatter(v: np.ndarray, r: int, h: int, w: int) -> np.ndarray:
    """For every pixel i, the sum of v_k over the centres k in K whose window holds i: v is (H-2r, W-2r[, ...])."""
    k = 2 * r + 1
    full = np.zeros((h + 2 * r, w + 2 * r) + v.shape[2:], v.dtype)
    full[2 * r:h, 2 * r:w] = v                    # centre k = (y, x) sits at (y + r, x + r) of the padded frame
    c = np.concatenate([np.zeros_like(full[:, :1]), full.cumsum(1)], axis=1)
    rows = c[:, k:] - c[:, :-k]
    c = np.concatenate([np.zeros_like(rows[:1]), rows.cumsum(0)], axis=0)
    return c[k:] - c[:-k]


def check_shape(h: int, w: int, r: int) -> None:
    if h < 2 * r + 1 or w < 2 * r + 1:
        raise ValueError(f"closed-form matte needs H, W >= 2r+1 = {2 * r + 1}, got {h}x{w}")


def window_stats(bgr: np.ndarray, r: int, eps: float):
    """(mu (H-2r, W-2r, 3), Delta^-1 (H-2r, W-2r, 3, 3)) of the windows in K, from exact integer window sums."""
    img = np.asarray(bgr, np.int64)
    h, w = img.shape[:2]
    check_shape(h, w, r)
    n = (2 * r + 1) ** 2
    s_i = _valid_box(img, r)
    s_ii = _valid_box(img[..., :, None] * img[..., None, :], r)
    sigma = (n * s_ii - s_i[..., :, None] * s_i[..., None, :]).astype(np.float64) / (65025.0 * n * n)
    mu = s_i / (255.0 * n)
    return mu, np.linalg.inv(sigma + (eps / n) * np.eye(3))


class Laplacian:
    """The matting Laplacian of one image in box-sum form."""

    def __init__(self, bgr: np.ndarray, r: int, eps: float):
        self.I = np.asarray(bgr, np.float64) / 255.0
        self.h, self.w = self.I.shape[:2]
        self.r, self.n = r, (2 * r + 1) ** 2
        self.mu, self.dinv = window_stats(bgr, r, eps)
        self.count = _scatter(np.ones(self.mu.shape[:2]), r, self.h, self.w)

    def apply(self, p: np.ndarray) -> np.ndarray:
        r, n = self.r, self.n
        p = np.asarray(p, np.float64)
        mp = _valid_box(p, r) / n
        mip = _valid_box(self.I * p[..., None], r) / n
        a = np.einsum("...ij,...j->...i", self.dinv, mip - self.mu * mp[..., None])
        b = mp - (a * self.mu).sum(-1)
        sa, sb = _scatter(a, r, self.h, self.w), _scatter(b, r, self.h, self.w)
        return self.count * p - ((sa * self.I).sum(-1) + sb)

    def diagonal(self) -> np.ndarray:
        """diag(L) from box sums of Delta^-1 (6 values), Delta^-1 mu (3) and mu^T Delta^-1 mu (1)."""
        r, n, I = self.r, self.n, self.I
        dm = np.einsum("...ij,...j->...i", self.dinv, self.mu)
        s_d = _scatter(self.dinv, r, self.h, self.w)
        s_dm = _scatter(dm, r, self.h, self.w)
        s_mdm = _scatter((self.mu * dm).sum(-1), r, self.h, self.w)
        quad = np.einsum("...i,...ij,...j->...", I, s_d, I) - 2.0 * (I * s_dm).sum(-1) + s_mdm
        return self.count * (1.0 - 1.0 / n) - quad / n


def laplacian_apply(bgr, p, r: int, eps: float) -> np.ndarray:
    return Laplacian(bgr, r, eps).apply(p)


def laplacian_diagonal(bgr, r: int, eps: float) -> np.ndarray:
    return Laplacian(bgr, r, eps).diagonal()


def dense_laplacian(bgr: np.ndarray, r: int, eps: float) -> np.ndarray:
    """L (HW x HW) assembled from its definition, one window at a time (tiny images only)."""
    I = np.asarray(bgr, np.float64).reshape(-1, 3) / 255.0
    h, w = bgr.shape[:2]
    check_shape(h, w, r)
    n = (2 * r + 1) ** 2
    L = np.zeros((h * w, h * w))
    for y in range(r, h - r):
        for x in range(r, w - r):
            idx = np.array([(y + dy) * w + (x + dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)])
            X = I[idx]
            mu = X.mean(0)
            sigma = (X - mu).T @ (X - mu) / n
            Xc = X - mu
            Lk = np.eye(n) - (1.0 + Xc @ np.linalg.inv(sigma + (eps / n) * np.eye(3)) @ Xc.T) / n
            L[np.ix_(idx, idx)] += Lk
    return L


def unknown_band(mask: np.ndarray, band: int) -> np.ndarray:
    return edge_band(mask, band)


def pcg(bgr: np.ndarray, mask: np.ndarray, r: int, eps: float, band: int, max_iter: int, tol: float):
    """Jacobi-preconditioned CG on L_UU alpha_U = -L_{U,known} m_known from alpha = m.
    -> (alpha (H, W) float64 unclamped, iterations, ||r_j|| / ||r_0||)."""
    m = (np.asarray(mask) != 0).astype(np.float64)
    U = unknown_band(mask, band)
    x = m.copy()
    if not U.any() or U.all():
        return x, 0, 0.0
    L = Laplacian(bgr, r, eps)
    dg = L.diagonal()[U]

    def op(v):
        p = np.zeros_like(m)
        p[U] = v
        return L.apply(p)[U]

    res = -L.apply(m)[U]
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


def direct_solve(bgr: np.ndarray, mask: np.ndarray, r: int, eps: float, band: int) -> np.ndarray:
    """The same system solved by numpy.linalg.solve on the dense L (tiny images only)."""
    m = (np.asarray(mask) != 0).astype(np.float64)
    U = unknown_band(mask, band).reshape(-1)
    L = dense_laplacian(bgr, r, eps)
    x = m.reshape(-1).copy()
    if U.any() and not U.all():
        x[U] = np.linalg.solve(L[np.ix_(U, U)], -L[np.ix_(U, ~U)] @ x[~U])
    return x.reshape(m.shape)


def residual_norms(bgr, mask, alpha_raw, r: int, eps: float, band: int):
    """(||(L alpha)_U||, ||(L m)_U||) in float64, the certificate the device's rel_residual is checked against."""
    m = (np.asarray(mask) != 0).astype(np.float64)
    U = unknown_band(mask, band)
    L = Laplacian(bgr, r, eps)
    return float(np.linalg.norm(L.apply(alpha_raw)[U])), float(np.linalg.norm(L.apply(m)[U]))


def strand_scene(h: int = 120, w: int = 160, radius: float = 40.0, ramp: float = 3.0, seed: int = 0):
    """A known matte with thin soft strands: soft_disk_scene's disk plus 12 radial strands, 1 or 2 px wide with alpha
    0.35..0.6, that start 8 px inside the disk's edge and end 14 px outside it, so they cross the edge.  Feathering the
    mask cannot bring them back.  -> (bgr u8, alpha* f64, mask u8 = alpha* >= 0.5)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
    d = np.hypot(yy - cy, xx - cx)
    alpha = np.clip((radius + ramp / 2.0 - d) / ramp, 0.0, 1.0)
    theta = np.arctan2(yy - cy, xx - cx)
    for s in range(12):
        ang = 2.0 * np.pi * (s + rng.uniform(0.2, 0.8)) / 12.0
        width = 1.0 if s % 2 == 0 else 2.0
        a_s = (0.35, 0.45, 0.55, 0.6)[s % 4]
        off = np.abs(np.sin(theta - ang)) * d                      # distance to the strand's ray
        on = (off <= width / 2.0) & (np.cos(theta - ang) > 0) & (d >= radius - 8.0) & (d <= radius + 14.0)
        alpha = np.where(on, np.maximum(alpha, a_s), alpha)
    fg, bg = _smooth_texture(rng, h, w, 150, 250), _smooth_texture(rng, h, w, 10, 110)
    img = np.rint(alpha[..., None] * fg + (1.0 - alpha[..., None]) * bg).astype(np.uint8)
    return img, alpha, (alpha >= 0.5).astype(np.uint8)


def band_sad(alpha, alpha_true, region) -> float:
    return float(np.abs(np.asarray(alpha, np.float64) - alpha_true)[region].sum())
