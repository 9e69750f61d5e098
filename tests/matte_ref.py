"""Float64 numpy restatement of the soft alpha matte (test infrastructure), written from He, Sun and Tang's equations
(Guided Image Filtering, TPAMI 2013, eqs. 19-20: the colour-guide filter), with guide I = bgr / 255, input p = mask != 0
and BORDER_REFLECT_101 windows of (2r+1)^2 pixels:

    a_k = (Sigma_k + eps U)^-1 (mean_k(I p) - mu_k mean_k(p)),   b_k = mean_k(p) - a_k . mu_k
    alpha_i = clip(mean_{k in w_i}(a_k) . I_i + mean_{k in w_i}(b_k), 0, 1)

Stage 1's window sums come from int64 integral images of the padded u8 inputs (exact); stage 2's from float64 sums over
the same padding.  brute_force_matte states the same thing as a per-pixel loop for tiny images."""
from __future__ import annotations

import numpy as np


def refl101(idx, n: int) -> np.ndarray:
    """BORDER_REFLECT_101 index map (period 2n - 2; any offset, so windows larger than the image work)."""
    idx = np.asarray(idx, np.int64)
    if n == 1:
        return np.zeros_like(idx)
    period = 2 * n - 2
    m = np.mod(idx, period)
    return np.where(m < n, m, period - m)


def _pad(a: np.ndarray, r: int) -> np.ndarray:
    h, w = a.shape[:2]
    return a[refl101(np.arange(-r, h + r), h)][:, refl101(np.arange(-r, w + r), w)]


def box_sum_int(a: np.ndarray, r: int) -> np.ndarray:
    """Exact (2r+1)^2 window sums of an integer array (H, W[, C]) from an int64 integral image."""
    h, w = a.shape[:2]
    k = 2 * r + 1
    p = _pad(a.astype(np.int64), r)
    ii = np.zeros((p.shape[0] + 1, p.shape[1] + 1) + p.shape[2:], np.int64)
    ii[1:, 1:] = p.cumsum(0).cumsum(1)
    return ii[k:k + h, k:k + w] - ii[:h, k:k + w] - ii[k:k + h, :w] + ii[:h, :w]


def box_sum_f64(a: np.ndarray, r: int) -> np.ndarray:
    """(2r+1)^2 window sums of a float array (H, W[, C]) in float64: row sums, then column sums of those."""
    h, w = a.shape[:2]
    k = 2 * r + 1
    p = _pad(a.astype(np.float64), r)
    c = np.concatenate([np.zeros_like(p[:, :1]), p.cumsum(1)], axis=1)
    rows = c[:, k:k + w] - c[:, :w]
    c = np.concatenate([np.zeros_like(rows[:1]), rows.cumsum(0)], axis=0)
    return c[k:k + h] - c[:h]


def matte_coefficients(bgr: np.ndarray, mask: np.ndarray, r: int, eps: float):
    """Stage 1: (a (H, W, 3), b (H, W)) per window centre, float64."""
    img = np.asarray(bgr, np.int64)
    p = (np.asarray(mask) != 0).astype(np.int64)
    n = (2 * r + 1) ** 2
    s_i = box_sum_int(img, r)                                          # (H, W, 3)
    s_ii = box_sum_int(img[..., :, None] * img[..., None, :], r)       # (H, W, 3, 3)
    s_p = box_sum_int(p, r)                                            # (H, W)
    s_ip = box_sum_int(img * p[..., None], r)                          # (H, W, 3)
    sigma = (n * s_ii - s_i[..., :, None] * s_i[..., None, :]).astype(np.float64) / (65025.0 * n * n)
    cov = (n * s_ip - s_i * s_p[..., None]).astype(np.float64) / (255.0 * n * n)
    a = np.linalg.solve(sigma + eps * np.eye(3), cov[..., None])[..., 0]
    b = s_p / n - (a * (s_i / (255.0 * n))).sum(-1)
    return a, b


def alpha_matte_ref(bgr: np.ndarray, mask: np.ndarray, r: int, eps: float) -> np.ndarray:
    """(H, W) float64 alpha in [0, 1]."""
    a, b = matte_coefficients(bgr, mask, r, eps)
    n = (2 * r + 1) ** 2
    ma, mb = box_sum_f64(a, r) / n, box_sum_f64(b, r) / n
    return np.clip((ma * (np.asarray(bgr, np.float64) / 255.0)).sum(-1) + mb, 0.0, 1.0)


def brute_force_matte(bgr: np.ndarray, mask: np.ndarray, r: int, eps: float) -> np.ndarray:
    """The same filter as an explicit loop over pixels and window taps (float64 means, no integral images)."""
    img = np.asarray(bgr, np.float64) / 255.0
    p = (np.asarray(mask) != 0).astype(np.float64)
    h, w = p.shape
    win = [[(refl101(np.arange(y - r, y + r + 1), h), refl101(np.arange(x - r, x + r + 1), w)) for x in range(w)]
           for y in range(h)]
    a = np.zeros((h, w, 3))
    b = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            ys, xs = win[y][x]
            iw = img[ys][:, xs].reshape(-1, 3)
            pw = p[ys][:, xs].reshape(-1)
            mu, pm = iw.mean(0), pw.mean()
            sigma = iw.T @ iw / len(pw) - np.outer(mu, mu)
            c = iw.T @ pw / len(pw) - mu * pm
            a[y, x] = np.linalg.solve(sigma + eps * np.eye(3), c)
            b[y, x] = pm - a[y, x] @ mu
    out = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            ys, xs = win[y][x]
            out[y, x] = a[ys][:, xs].reshape(-1, 3).mean(0) @ img[y, x] + b[ys][:, xs].mean()
    return np.clip(out, 0.0, 1.0)


def grey_guided_filter(guide: np.ndarray, src: np.ndarray, r: int, eps: float) -> np.ndarray:
    """He et al.'s grey-guide filter in float64 with the same windows (unclamped)."""
    n = (2 * r + 1) ** 2
    g, s = np.asarray(guide, np.float64), np.asarray(src, np.float64)
    mean = lambda v: box_sum_f64(v, r) / n                              # noqa: E731
    mg, ms = mean(g), mean(s)
    a = (mean(g * s) - mg * ms) / (mean(g * g) - mg * mg + eps)
    b = ms - a * mg
    return mean(a) * g + mean(b)


def _smooth_texture(rng, h: int, w: int, lo: int, hi: int) -> np.ndarray:
    """A low-frequency colour texture in [lo, hi]: a random grid every 10 pixels, bilinearly interpolated."""
    g = rng.uniform(lo, hi, size=(h // 10 + 2, w // 10 + 2, 3))
    ys, xs = np.linspace(0.0, g.shape[0] - 1.001, h), np.linspace(0.0, g.shape[1] - 1.001, w)
    y0, x0 = ys.astype(np.int64), xs.astype(np.int64)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    return (g[y0][:, x0] * (1 - fy) * (1 - fx) + g[y0][:, x0 + 1] * (1 - fy) * fx + g[y0 + 1][:, x0] * fy * (1 - fx)
            + g[y0 + 1][:, x0 + 1] * fy * fx)


def soft_disk_scene(h: int = 120, w: int = 160, radius: float = 40.0, ramp: float = 3.0, seed: int = 0):
    """A known matte: I = round(alpha* F + (1 - alpha*) B) with low-frequency textures F in [150, 250] and B in [10, 110]
    (disjoint colour ranges) and alpha* a disk whose edge is a linear ramp `ramp` pixels wide.
    -> (bgr u8, alpha* f64, mask u8 = alpha* >= 0.5)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.hypot(yy - (h - 1) / 2.0, xx - (w - 1) / 2.0)
    alpha = np.clip((radius + ramp / 2.0 - d) / ramp, 0.0, 1.0)
    fg, bg = _smooth_texture(rng, h, w, 150, 250), _smooth_texture(rng, h, w, 10, 110)
    img = np.rint(alpha[..., None] * fg + (1.0 - alpha[..., None]) * bg).astype(np.uint8)
    return img, alpha, (alpha >= 0.5).astype(np.uint8)


def edge_band(mask: np.ndarray, width: int) -> np.ndarray:
    """Pixels within Chebyshev distance `width` of a pixel whose 8-neighbourhood holds both mask values."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    pad = np.pad(m, 1, mode="edge")
    lo, hi = np.ones_like(m), np.zeros_like(m)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            v = pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            lo, hi = lo & v, hi | v
    edge = (hi & ~lo).astype(np.int64)
    ii = np.zeros((h + 1, w + 1), np.int64)
    ii[1:, 1:] = edge.cumsum(0).cumsum(1)
    y0 = np.clip(np.arange(h) - width, 0, h)
    y1 = np.clip(np.arange(h) + width + 1, 0, h)
    x0 = np.clip(np.arange(w) - width, 0, w)
    x1 = np.clip(np.arange(w) + width + 1, 0, w)
    cnt = ii[y1][:, x1] - ii[y0][:, x1] - ii[y1][:, x0] + ii[y0][:, x0]
    return cnt > 0
