"""Float64 / int64 numpy restatement of the four matte errors of Rhemann et al. (CVPR 2009) as include/ggc.h defines
them for ggc_matte_errors (test infrastructure).  Inputs are 8-bit alpha levels a (the matte under test) and g (the true
matte); `region` (nonzero = counted) restricts the sums only.

    SAD  = sum_R |a - g|                SSE = sum_R (a - g)^2                                    (integers)
    CONN = sum_R |D(10 a - 255 lev) - D(10 g - 255 lev)|, D(d) = d if d >= 383 else 0            (integer)
           lev(p) = (the first k in 1..10 with p outside Omega_k) - 1, 10 if there is none; Omega_k the largest
           4-connected component of {10 a >= 255 k} & {10 g >= 255 k}, ties to the smallest raster index
    GRAD = sum_R (m(a) - m(g))^2, m the magnitude of the 9 x 9 Gaussian-derivative responses (sigma 1.4), border replicated

matte_errors_ref uses scipy.ndimage (label, correlate); brute_force_errors states the same thing with a plain BFS and an
81-tap double loop, for tiny images."""
from __future__ import annotations

from collections import deque

import numpy as np
from scipy import ndimage

SIGMA = 1.4
HALF = 4
THETA_D = 383          # d / 2550 >= 0.15
LEVELS = 10


def taps():
    """(G, G') at x = -4..4, float64."""
    x = np.arange(-HALF, HALF + 1, dtype=np.float64)
    g = np.exp(-x * x / (2.0 * SIGMA * SIGMA)) / (SIGMA * np.sqrt(2.0 * np.pi))
    return g, -x * g / (SIGMA * SIGMA)


def filters():
    """(F_x, F_y), 9 x 9: F_x[i][j] = G(i) G'(j) / N, rows i, columns j; F_y its transpose."""
    g, d = taps()
    fx = np.outer(g, d)
    fx = fx / np.sqrt((fx * fx).sum())
    return fx, fx.T.copy()


def gradient_magnitude(levels: np.ndarray) -> np.ndarray:
    u = np.asarray(levels, np.float64) / 255.0
    fx, fy = filters()
    rx = ndimage.correlate(u, fx, mode="nearest")
    ry = ndimage.correlate(u, fy, mode="nearest")
    return np.sqrt(rx * rx + ry * ry)


def threshold_set(a: np.ndarray, g: np.ndarray, k: int) -> np.ndarray:
    return (10 * a.astype(np.int64) >= 255 * k) & (10 * g.astype(np.int64) >= 255 * k)


def largest_component(s: np.ndarray) -> np.ndarray:
    """The largest 4-connected component of a boolean image, ties to the one holding the smallest raster index."""
    lab, n = ndimage.label(s, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    if n == 0:
        return np.zeros_like(s, dtype=bool)
    first = np.full(n + 1, s.size, np.int64)                     # smallest raster index per label
    np.minimum.at(first, lab.ravel(), np.arange(s.size))
    area = np.bincount(lab.ravel(), minlength=n + 1)
    best = max(range(1, n + 1), key=lambda c: (area[c], -first[c]))
    return lab == best


def connectivity_levels(a: np.ndarray, g: np.ndarray) -> np.ndarray:
    lev = np.full(a.shape, LEVELS, np.uint8)
    alive = np.ones(a.shape, bool)
    for k in range(1, LEVELS + 1):
        omega = largest_component(threshold_set(a, g, k))
        lev[alive & ~omega] = k - 1
        alive &= omega
    return lev


def _conn_d(d: np.ndarray) -> np.ndarray:
    return np.where(d >= THETA_D, d, 0)


def _sums(a, g, region, lev, ma, mg) -> dict:
    a, g = a.astype(np.int64), g.astype(np.int64)
    r = np.ones(a.shape, bool) if region is None else np.asarray(region) != 0
    l = lev.astype(np.int64)
    da, dg = 10 * a - 255 * l, 10 * g - 255 * l
    assert (da >= 0).all() and (dg >= 0).all()
    e = np.abs(a - g)
    return dict(n=int(r.sum()), sad=int(e[r].sum()), sse=int((e * e)[r].sum()),
                conn=int(np.abs(_conn_d(da) - _conn_d(dg))[r].sum()),
                grad=float(((ma - mg) ** 2)[r].sum()), levels=lev)


def matte_errors_ref(a: np.ndarray, g: np.ndarray, region=None) -> dict:
    """-> dict(n, sad, sse, conn: int; grad: float (the raw sums of the entry); levels: (H, W) uint8)."""
    a, g = np.asarray(a), np.asarray(g)
    assert a.dtype == np.uint8 and g.dtype == np.uint8 and a.shape == g.shape and a.ndim == 2
    return _sums(a, g, region, connectivity_levels(a, g), gradient_magnitude(a), gradient_magnitude(g))


def conventional(e: dict) -> dict:
    """The raw sums in the units the benchmarks report."""
    n = e["n"]
    return dict(sad=e["sad"] / 255.0 / 1000.0, mse=e["sse"] / 65025.0 / n if n else 0.0, grad=e["grad"] / 1000.0,
                conn=e["conn"] / 2550.0 / 1000.0, n_pixels=n)


# ---------------------------------------------------------------- the same, by loops
def _bfs_largest(s: np.ndarray) -> set:
    h, w = s.shape
    seen = np.zeros((h, w), bool)
    best: list = []
    for y in range(h):                                           # raster order: a later component must be strictly larger
        for x in range(w):
            if not s[y, x] or seen[y, x]:
                continue
            comp, todo = [], deque([(y, x)])
            seen[y, x] = True
            while todo:
                cy, cx = todo.popleft()
                comp.append((cy, cx))
                for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                    if 0 <= ny < h and 0 <= nx < w and s[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        todo.append((ny, nx))
            if len(comp) > len(best):
                best = comp
    return set(best)


def _loop_magnitude(levels: np.ndarray) -> np.ndarray:
    g, d = taps()
    norm = np.sqrt(sum((g[i] * d[j]) ** 2 for i in range(9) for j in range(9)))
    h, w = levels.shape
    out = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            rx = ry = 0.0
            for i in range(-HALF, HALF + 1):
                for j in range(-HALF, HALF + 1):
                    u = float(levels[min(max(y + i, 0), h - 1), min(max(x + j, 0), w - 1)]) / 255.0
                    rx += g[i + HALF] * d[j + HALF] / norm * u
                    ry += d[i + HALF] * g[j + HALF] / norm * u
            out[y, x] = np.sqrt(rx * rx + ry * ry)
    return out


def brute_force_errors(a: np.ndarray, g: np.ndarray, region=None) -> dict:
    a, g = np.asarray(a), np.asarray(g)
    h, w = a.shape
    lev = np.full((h, w), LEVELS, np.uint8)
    omegas = [_bfs_largest(threshold_set(a, g, k)) for k in range(1, LEVELS + 1)]
    for y in range(h):
        for x in range(w):
            for k in range(1, LEVELS + 1):
                if (y, x) not in omegas[k - 1]:
                    lev[y, x] = k - 1
                    break
    return _sums(a, g, region, lev, _loop_magnitude(a), _loop_magnitude(g))


# ---------------------------------------------------------------- shared cases
def to_levels(alpha) -> np.ndarray:
    """floor(255 alpha + 0.5) as uint8: pipeline.alpha_to_u8 without the package."""
    return np.floor(np.asarray(alpha, np.float64) * 255.0 + 0.5).astype(np.uint8)


def tie_case():
    """The 5 x 9 case of two equal squares: -> (a, g).  SAD 408, SSE 41616, CONN 4080, n 45."""
    g = np.zeros((5, 9), np.uint8)
    g[1:3, 1:3] = 255
    g[1:3, 5:7] = 255
    a = g.copy()
    a[1:3, 5:7] = 153
    return a, g


def random_levels(rng, h: int, w: int) -> np.ndarray:
    """Uniform-random levels in which every threshold k = 1..10 has pixels (where the image has room for them)."""
    v = rng.integers(0, 256, (h, w)).astype(np.uint8)
    flat = v.ravel()
    picks = [26, 51, 77, 102, 128, 153, 179, 204, 230, 255]          # ceil(25.5 k)
    for i, p in enumerate(picks[:flat.size]):
        flat[(i * 7919) % flat.size] = p
    return v


def blocky_levels(rng, h: int, w: int, block: int = 3) -> np.ndarray:
    """Blocks of equal size on a zero background, separated by gaps, with levels from a few values: equal-area ties."""
    v = np.zeros((h, w), np.uint8)
    vals = np.array([0, 77, 153, 204, 255], np.uint8)
    for y in range(0, h - block + 1, block + 1):
        for x in range(0, w - block + 1, block + 1):
            v[y:y + block, x:x + block] = vals[rng.integers(0, len(vals))]
    return v


def fading_levels(h: int, w: int, top: int) -> np.ndarray:
    """A horizontal ramp whose largest level is `top`: S_k is empty for every k with 255 k > 10 top."""
    return np.broadcast_to(np.linspace(0, top, w).astype(np.uint8), (h, w)).copy()
