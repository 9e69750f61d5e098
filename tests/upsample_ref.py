"""Float64 numpy restatement of the full-resolution matte (test infrastructure): the fast guided filter (He and Sun,
"Fast Guided Filter", 2015) over the colour guided filter of matte_ref.py.

    stage 2':  C = (mean a / 255, mean b) per working pixel, (H, W, 4)      (matte_ref's stages 1-2, by import)
    stage 3:   per output pixel (y, x) of (H1, W1): sx = ((x + 0.5) * W) / W1 - 0.5, raised to 0; x0 = floor(sx), and
               x0 = W - 1 with wx = 0 when x0 >= W - 1, else wx = sx - x0; x1 = min(x0 + 1, W - 1); the same for y.
               c = lerp(lerp(C[y0,x0], C[y0,x1], wx), lerp(C[y1,x0], C[y1,x1], wx), wy), lerp(u, v, t) = u + t (v - u)
               alpha = clip(c0 B + c1 G + c2 R + c3, 0, 1) with the full-resolution bytes

brute_force_upsample states the same per pixel, with window means by explicit loops, for tiny images."""
from __future__ import annotations

import math

import numpy as np

from matte_ref import box_sum_f64, matte_coefficients, refl101


def source_coords(n1: int, n: int):
    """(i0, i1, w) for every output index 0..n1-1 over a source of n, as int64 / float64 arrays."""
    s = ((np.arange(n1, dtype=np.float64) + 0.5) * n) / n1 - 0.5
    s = np.where(s < 0.0, 0.0, s)
    f = np.floor(s)
    i0 = f.astype(np.int64)
    last = i0 >= n - 1
    w = np.where(last, 0.0, s - f)
    i0 = np.where(last, n - 1, i0)
    return i0, np.minimum(i0 + 1, n - 1), w


def mean_coefficients(bgr: np.ndarray, mask: np.ndarray, r: int, eps: float) -> np.ndarray:
    """Stage 2': (H, W, 4) float64 = (mean a0 / 255, mean a1 / 255, mean a2 / 255, mean b)."""
    a, b = matte_coefficients(bgr, mask, r, eps)
    n = (2 * r + 1) ** 2
    return np.concatenate([box_sum_f64(a, r) / n / 255.0, (box_sum_f64(b, r) / n)[..., None]], axis=2)


def _lerp(u, v, t):
    return u + t * (v - u)


def apply_coefficients(c: np.ndarray, full: np.ndarray) -> np.ndarray:
    """Stage 3: the (H, W, 4) coefficients interpolated to full's (H1, W1) and applied to its bytes -> alpha (H1, W1)."""
    h, w = c.shape[:2]
    h1, w1 = full.shape[:2]
    y0, y1, wy = source_coords(h1, h)
    x0, x1, wx = source_coords(w1, w)
    wx3 = wx[None, :, None]
    top = _lerp(c[y0][:, x0], c[y0][:, x1], wx3)
    bot = _lerp(c[y1][:, x0], c[y1][:, x1], wx3)
    cc = _lerp(top, bot, wy[:, None, None])
    f = np.asarray(full, np.float64)
    a = cc[..., 0] * f[..., 0] + cc[..., 1] * f[..., 1] + cc[..., 2] * f[..., 2] + cc[..., 3]
    return np.clip(a, 0.0, 1.0)


def upsample_ref(bgr: np.ndarray, mask: np.ndarray, full: np.ndarray, r: int, eps: float) -> np.ndarray:
    """(H1, W1) float64 alpha."""
    return apply_coefficients(mean_coefficients(bgr, mask, r, eps), full)


def _coord(o: int, n1: int, n: int):
    s = ((o + 0.5) * n) / n1 - 0.5
    s = max(s, 0.0)
    i0 = math.floor(s)
    if i0 >= n - 1:
        return n - 1, n - 1, 0.0
    return i0, min(i0 + 1, n - 1), s - i0


def brute_force_upsample(bgr: np.ndarray, mask: np.ndarray, full: np.ndarray, r: int, eps: float) -> np.ndarray:
    """The same as a loop over pixels and window taps: per-window (a, b) by a 3x3 solve of explicit means, their window
    means per working pixel, then per output pixel the four corners and the lerps in Python floats."""
    img = np.asarray(bgr, np.float64) / 255.0
    p = (np.asarray(mask) != 0).astype(np.float64)
    h, w = p.shape
    win = lambda y, x: (refl101(np.arange(y - r, y + r + 1), h), refl101(np.arange(x - r, x + r + 1), w))  # noqa: E731
    a = np.zeros((h, w, 3))
    b = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            ys, xs = win(y, x)
            iw = img[ys][:, xs].reshape(-1, 3)
            pw = p[ys][:, xs].reshape(-1)
            mu, pm = iw.mean(0), pw.mean()
            sigma = iw.T @ iw / len(pw) - np.outer(mu, mu)
            a[y, x] = np.linalg.solve(sigma + eps * np.eye(3), iw.T @ pw / len(pw) - mu * pm)
            b[y, x] = pm - a[y, x] @ mu
    c = np.zeros((h, w, 4))
    for y in range(h):
        for x in range(w):
            ys, xs = win(y, x)
            c[y, x, :3] = a[ys][:, xs].reshape(-1, 3).mean(0) / 255.0
            c[y, x, 3] = b[ys][:, xs].mean()
    f = np.asarray(full, np.float64)
    h1, w1 = f.shape[:2]
    out = np.zeros((h1, w1))
    for y in range(h1):
        ya, yb, wy = _coord(y, h1, h)
        for x in range(w1):
            xa, xb, wx = _coord(x, w1, w)
            k = [_lerp(_lerp(c[ya, xa, i], c[ya, xb, i], wx), _lerp(c[yb, xa, i], c[yb, xb, i], wx), wy) for i in range(4)]
            out[y, x] = min(max(k[0] * f[y, x, 0] + k[1] * f[y, x, 1] + k[2] * f[y, x, 2] + k[3], 0.0), 1.0)
    return out


def resize_bgr(img: np.ndarray, h1: int, w1: int) -> np.ndarray:
    """A larger image of the same scene for the tests: bilinear (half-pixel centres) with a little seeded noise, u8."""
    y0, y1, wy = source_coords(h1, img.shape[0])
    x0, x1, wx = source_coords(w1, img.shape[1])
    f = np.asarray(img, np.float64)
    top = _lerp(f[y0][:, x0], f[y0][:, x1], wx[None, :, None])
    bot = _lerp(f[y1][:, x0], f[y1][:, x1], wx[None, :, None])
    out = _lerp(top, bot, wy[:, None, None])
    noise = np.random.default_rng(h1 * 7 + w1).integers(-3, 4, out.shape)
    return np.clip(np.rint(out) + noise, 0, 255).astype(np.uint8)


def far_field(mask: np.ndarray, r: int, h1: int, w1: int) -> np.ndarray:
    """(H1, W1) bool: output pixels whose four source pixels all lie farther than 2r (Chebyshev) from every change of
    the mask, i.e. outside matte_ref.edge_band(mask, 2r)."""
    from matte_ref import edge_band
    far = ~edge_band(mask, 2 * r)
    y0, y1, _ = source_coords(h1, mask.shape[0])
    x0, x1, _ = source_coords(w1, mask.shape[1])
    return far[y0][:, x0] & far[y0][:, x1] & far[y1][:, x0] & far[y1][:, x1]
