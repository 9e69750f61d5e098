"""A numpy / scipy restatement of include/ggc.h O5 and O6: the integer alpha-over, and gradient-domain cloning (Perez,
Gangnet and Blake, SIGGRAPH 2003) with source or mixed gradients.  The system is assembled with integer right-hand
sides; `exact` solves it by sparse LU, `pcg` by the float64 preconditioned CG of the definition.  Nothing here is shared
with the library: the tests compare the two."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

FLOOR = 2.55e-10                                  # the absolute floor on ||r||, per sqrt of an unknown
STEPS = ((-1, 0), (0, -1), (0, 1), (1, 0))


def over(rgba, background, offset):
    """(a c + (255 - a) bg + 127) // 255 where the cut-out covers the background, the background elsewhere."""
    out = background.copy()
    hs, ws = rgba.shape[:2]
    h, w = background.shape[:2]
    r, c = int(offset[0]), int(offset[1])
    y0, y1, x0, x1 = max(r, 0), min(r + hs, h), max(c, 0), min(c + ws, w)
    if y0 >= y1 or x0 >= x1:
        return out
    cut = rgba[y0 - r:y1 - r, x0 - c:x1 - c].astype(np.int64)
    a = cut[..., 3:4]
    bg = background[y0:y1, x0:x1].astype(np.int64)
    out[y0:y1, x0:x1] = ((a * cut[..., :3] + (255 - a) * bg + 127) // 255).astype(np.uint8)
    return out


def on_target(source, mask, target_shape, offset):
    """The source carried to the target's frame: g (H,W,3) int64 (0 where no source pixel exists), has (H,W) bool = the
    source pixel exists, omega (H,W) bool = it exists and is selected."""
    h, w = target_shape[:2]
    hs, ws = mask.shape
    g = np.zeros((h, w, 3), np.int64)
    has = np.zeros((h, w), bool)
    omega = np.zeros((h, w), bool)
    r, c = int(offset[0]), int(offset[1])
    y0, y1, x0, x1 = max(r, 0), min(r + hs, h), max(c, 0), min(c + ws, w)
    if y0 < y1 and x0 < x1:
        g[y0:y1, x0:x1] = source[y0 - r:y1 - r, x0 - c:x1 - c]
        has[y0:y1, x0:x1] = True
        omega[y0:y1, x0:x1] = mask[y0 - r:y1 - r, x0 - c:x1 - c] != 0
    return g, has, omega


def _shift(a, dy, dx, fill=0):
    """b[y, x] = a[y + dy, x + dx], `fill` where that lies outside."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    b[yd, xd] = a[ys, xs]
    return b


def assemble(source, mask, target, offset, mixed):
    """-> dict(omega (H,W) bool, A csr [n,n], b (n,3) int64, deg (n,) int64, g (n,3) int64): the system of the
    definition on Omega's pixels in raster order, and the start f = g."""
    h, w = target.shape[:2]
    g, has, omega = on_target(source, mask, target.shape, offset)
    t = target.astype(np.int64)
    inside = np.ones((h, w), bool)
    idx = np.full((h, w), -1, np.int64)
    n = int(omega.sum())
    idx[omega] = np.arange(n)
    deg = np.zeros((h, w), np.int64)
    rhs = np.zeros((h, w, 3), np.int64)
    rows, cols = [], []
    for dy, dx in STEPS:
        q_in = _shift(inside, dy, dx, False)                       # q = p + step lies inside the target
        q_om, q_has = _shift(omega, dy, dx, False), _shift(has, dy, dx, False)
        gq, tq = _shift(g, dy, dx), _shift(t, dy, dx)
        deg += q_in
        ds = np.where(q_has[..., None], g - gq, 0)
        dt = t - tq
        v = np.where(np.abs(dt) > np.abs(ds), dt, ds) if mixed else ds
        rhs += np.where(q_in[..., None], v, 0) + np.where((q_in & ~q_om)[..., None], tq, 0)
        link = omega & q_om
        rows.append(idx[link])
        cols.append(_shift(idx, dy, dx, -1)[link])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    d = deg[omega]
    A = sp.csr_matrix((np.concatenate([d.astype(np.float64), -np.ones(len(rows))]),
                       (np.concatenate([np.arange(n), rows]), np.concatenate([np.arange(n), cols]))), shape=(n, n))
    return dict(omega=omega, A=A, b=rhs[omega], deg=d, g=g[omega])


def exact(sys):
    """The solution by sparse LU, (n,3) float64."""
    A = sys["A"].tocsc()
    return np.stack([spsolve(A, sys["b"][:, ch].astype(np.float64)) for ch in range(3)], axis=1).reshape(-1, 3)


def first_residual(sys):
    """r_0 = b - A g in exact integers, (n,3) int64."""
    Ai = sys["A"].astype(np.int64)
    return sys["b"] - Ai @ sys["g"]


def pcg(sys, max_iter, tol):
    """The float64 PCG of the definition, one CG over the three channels: Jacobi preconditioner |N_p|, start f = g, stop
    when ||r|| <= max(tol ||r_0||, FLOOR sqrt(3 n)), tested on r_0 too.  -> (f (n,3), iterations, ||r|| / ||r_0||)."""
    A, d = sys["A"], sys["deg"].astype(np.float64)[:, None]
    f = sys["g"].astype(np.float64)
    r = first_residual(sys).astype(np.float64)
    r0 = np.sqrt((r * r).sum())
    stop = max(tol * r0, FLOOR * np.sqrt(3.0 * len(f)))
    if not r0 > stop:
        return f, 0, 0.0
    z = r / d
    p, rz = z.copy(), (r * z).sum()
    it, rel = 0, 0.0
    while it < max_iter:
        q = A @ p
        pq = (p * q).sum()
        if not (pq > 0 and np.isfinite(pq)):
            break
        al = rz / pq
        f += al * p
        r -= al * q
        it += 1
        rn = np.sqrt((r * r).sum())
        rel = rn / r0
        if rn <= stop:
            break
        z = r / d
        rz_new = (r * z).sum()
        p = z + (rz_new / rz) * p
        rz = rz_new
    return f, it, rel


def residual_norms(sys, raw):
    """(||b - A f||, ||r_0||) in float64 for f = raw (H,W,3) on Omega."""
    r = sys["b"].astype(np.float64) - sys["A"] @ raw[sys["omega"]]
    r0 = first_residual(sys).astype(np.float64)
    return float(np.sqrt((r * r).sum())), float(np.sqrt((r0 * r0).sum()))


def to_bytes(f):
    """floor(clamp(f, 0, 255) + 0.5)"""
    return np.floor(np.clip(f, 0.0, 255.0) + 0.5).astype(np.uint8)


def clone(source, mask, target, offset, mixed, max_iter, tol, solve="pcg"):
    """The whole rule -> dict(composite (H,W,3) uint8, raw (H,W,3) float64, n_omega, iters, rel).  An image whose Omega
    is empty or the whole target is not solved: the target, or the pasted source."""
    sys = assemble(source, mask, target, offset, mixed)
    om, n = sys["omega"], len(sys["g"])
    raw = target.astype(np.float64)
    it, rel = 0, 0.0
    if n == om.size:
        raw[om] = sys["g"]
    elif n > 0:
        if solve == "pcg":
            f, it, rel = pcg(sys, max_iter, tol)
        else:
            f = exact(sys)
        raw[om] = f
    comp = target.copy()
    comp[om] = to_bytes(raw[om])
    return dict(composite=comp, raw=raw, n_omega=n, iters=it, rel=rel, omega=om)
