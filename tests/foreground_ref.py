"""Float64 numpy restatement of the foreground colour estimation (test infrastructure), written from the definition in
include/ggc.h (entry O4): the multi-level foreground estimation energy of Germer, Uelwer, Conrad and Harmeling ("Fast
Multi-Level Foreground Estimation", ICPR 2020) restricted to the pixels of fractional alpha, with Dirichlet values.

Per image and colour channel, I = bgr / 255, a = snap(alpha), U = {0 < a < 1}, O = {a = 1}, Z = {a = 0}:

    E = sum_U (a F + (1 - a) B - I)^2 + DELTA sum_U [(F - I)^2 + (B - I)^2]
      + sum_(i,j) w_ij [phiF_ij (F_i - F_j)^2 + phiB_ij (B_i - B_j)^2],   w_ij = eps_r + omega |a_i - a_j|

over the 4-neighbour pairs with an end in U; phiF = 1 when both ends are in U or O (F = I on O), phiB = 1 when both
are in U or Z (B = I on Z).  `System` holds the links, `apply` is the homogeneous operator A, `gradient` is A x - b for
full-frame F, B (known pixels at I), `pcg` the block-Jacobi preconditioned CG of the definition, `dense_solve` the same
system through numpy.linalg.solve for tiny images."""
from __future__ import annotations

import numpy as np

from closed_form_ref import strand_scene
from matte_ref import _smooth_texture, soft_disk_scene

DELTA = 1e-6
SNAP = 1.0 / 510.0
ABS_FLOOR = 1e-12


def snap(alpha) -> np.ndarray:
    """alpha' of the definition: 0 below 1/510, 1 above 1 - 1/510 (the pixels whose alpha byte is 0 or 255); a NaN is
    snapped to 0 (it is not >= 1/510)."""
    a = np.array(alpha, np.float64)
    out = a.copy()
    out[~(a >= SNAP)] = 0.0
    out[a > 1.0 - SNAP] = 1.0
    return out


class System:
    """The linear system of one image: alpha' (already snapped), the sets, the link weights."""

    def __init__(self, bgr, alpha_snapped, eps_r: float, omega: float):
        a = np.asarray(alpha_snapped, np.float64)
        self.a = a
        self.I = np.asarray(bgr, np.float64) / 255.0
        self.U = (a > 0.0) & (a < 1.0)
        one, zero = a >= 1.0, a <= 0.0
        self.links = []
        for ax in (0, 1):
            s0 = tuple(slice(0, -1) if k == ax else slice(None) for k in range(2))
            s1 = tuple(slice(1, None) if k == ax else slice(None) for k in range(2))
            w = eps_r + omega * np.abs(a[s0] - a[s1])
            any_u = self.U[s0] | self.U[s1]
            ff = any_u & (self.U[s0] | one[s0]) & (self.U[s1] | one[s1])
            fb = any_u & (self.U[s0] | zero[s0]) & (self.U[s1] | zero[s1])
            self.links.append((s0, s1, w * ff, w * fb))
        dff, dbb = a * a + DELTA, (1.0 - a) ** 2 + DELTA
        for s0, s1, wf, wb in self.links:
            dff[s0] += wf
            dff[s1] += wf
            dbb[s0] += wb
            dbb[s1] += wb
        self.dff, self.dbb, self.dfb = dff, dbb, a * (1.0 - a)

    def _smooth(self, F, B, oF, oB):
        for s0, s1, wf, wb in self.links:
            dF = (F[s0] - F[s1]) * wf[..., None]
            dB = (B[s0] - B[s1]) * wb[..., None]
            oF[s0] += dF
            oF[s1] -= dF
            oB[s0] += dB
            oB[s1] -= dB
        oF[~self.U] = 0.0
        oB[~self.U] = 0.0
        return oF, oB

    def apply(self, F, B):
        """A [F; B] for full-frame (H,W,3) arrays that are zero off U (the homogeneous operator)."""
        a = self.a[..., None]
        m = a * F + (1.0 - a) * B
        return self._smooth(F, B, a * m + DELTA * F, (1.0 - a) * m + DELTA * B)

    def gradient(self, F, B):
        """A x - b = half the gradient of E at full-frame F, B that hold I off U."""
        a = self.a[..., None]
        m = a * F + (1.0 - a) * B - self.I
        return self._smooth(F, B, a * m + DELTA * (F - self.I), (1.0 - a) * m + DELTA * (B - self.I))

    def energy(self, F, B) -> float:
        a, U = self.a[..., None], self.U
        e = (((a * F + (1.0 - a) * B - self.I) ** 2)[U]).sum()
        e += DELTA * ((((F - self.I) ** 2)[U]).sum() + (((B - self.I) ** 2)[U]).sum())
        for s0, s1, wf, wb in self.links:
            e += (wf[..., None] * (F[s0] - F[s1]) ** 2).sum() + (wb[..., None] * (B[s0] - B[s1]) ** 2).sum()
        return float(e)

    def precondition(self, rF, rB):
        """The exact 2 x 2 diagonal block of every pixel of U, inverted."""
        det = (self.dff * self.dbb - self.dfb * self.dfb)[..., None]
        zF = (self.dbb[..., None] * rF - self.dfb[..., None] * rB) / det
        zB = (self.dff[..., None] * rB - self.dfb[..., None] * rF) / det
        u = self.U[..., None]
        return zF * u, zB * u


def _dot(aF, aB, bF, bB) -> float:
    return float((aF * bF).sum() + (aB * bB).sum())


def pcg(bgr, alpha_snapped, eps_r: float, omega: float, max_iter: int, tol: float):
    """Preconditioned CG from F = B = I, one CG over the three channels.
    -> (F, B (H,W,3) float64 unclamped, I off U; iterations; ||r_j|| / ||r_0||, 0.0 with 0 iterations)."""
    s = System(bgr, alpha_snapped, eps_r, omega)
    F, B = s.I.copy(), s.I.copy()
    gF, gB = s.gradient(F, B)
    rF, rB = -gF, -gB
    r0 = np.sqrt(_dot(rF, rB, rF, rB))
    stop = max(tol * r0, ABS_FLOOR * np.sqrt(6.0 * s.U.sum()))
    if not s.U.any() or r0 <= stop:
        return F, B, 0, 0.0
    zF, zB = s.precondition(rF, rB)
    pF, pB = zF.copy(), zB.copy()
    rz = _dot(rF, rB, zF, zB)
    it, rn = 0, r0
    while it < max_iter:
        qF, qB = s.apply(pF, pB)
        al = rz / _dot(pF, pB, qF, qB)
        F += al * pF
        B += al * pB
        rF -= al * qF
        rB -= al * qB
        it += 1
        rn = np.sqrt(_dot(rF, rB, rF, rB))
        if rn <= stop:
            break
        zF, zB = s.precondition(rF, rB)
        rz_new = _dot(rF, rB, zF, zB)
        pF = zF + (rz_new / rz) * pF
        pB = zB + (rz_new / rz) * pB
        rz = rz_new
    return F, B, it, rn / r0


def dense_matrix(bgr, alpha_snapped, eps_r: float, omega: float):
    """(A (6|U| x 6|U|), b) assembled column by column from `apply` and `gradient` (tiny images only); unknown order:
    F then B, each (pixel of U in raster order, channel)."""
    s = System(bgr, alpha_snapped, eps_r, omega)
    n = int(s.U.sum()) * 3
    A = np.zeros((2 * n, 2 * n))
    for k in range(2 * n):
        F, B = np.zeros_like(s.I), np.zeros_like(s.I)
        e = np.zeros(n)
        e[k % n] = 1.0
        (F if k < n else B)[s.U] = e.reshape(-1, 3)
        oF, oB = s.apply(F, B)
        A[:, k] = np.concatenate([oF[s.U].reshape(-1), oB[s.U].reshape(-1)])
    gF, gB = s.gradient(s.I.copy(), s.I.copy())
    x0 = np.concatenate([s.I[s.U].reshape(-1), s.I[s.U].reshape(-1)])
    b = A @ x0 - np.concatenate([gF[s.U].reshape(-1), gB[s.U].reshape(-1)])
    return A, b, s


def dense_solve(bgr, alpha_snapped, eps_r: float, omega: float):
    """The same system through numpy.linalg.solve -> (F, B) full frame, I off U."""
    A, b, s = dense_matrix(bgr, alpha_snapped, eps_r, omega)
    F, B = s.I.copy(), s.I.copy()
    if s.U.any():
        x = np.linalg.solve(A, b)
        n = len(x) // 2
        F[s.U] = x[:n].reshape(-1, 3)
        B[s.U] = x[n:].reshape(-1, 3)
    return F, B


def residual_norms(bgr, alpha_snapped, eps_r: float, omega: float, F, B):
    """(||A x - b|| at F, B; ||A x - b|| at F = B = I) in float64: the certificate the device's rel_residual is held to."""
    s = System(bgr, alpha_snapped, eps_r, omega)
    F, B = np.array(F, np.float64), np.array(B, np.float64)
    F[~s.U] = s.I[~s.U]
    B[~s.U] = s.I[~s.U]
    gF, gB = s.gradient(F, B)
    g0F, g0B = s.gradient(s.I.copy(), s.I.copy())
    return float(np.sqrt(_dot(gF, gB, gF, gB))), float(np.sqrt(_dot(g0F, g0B, g0F, g0B)))


def scene_colours(kind: str, seed: int, h: int = 120, w: int = 160):
    """soft_disk_scene(h, w, 40, 3, seed) ("disk") or strand_scene(h, w, seed=seed) ("strands") with the true colours:
    the scene's generator replayed.  -> (bgr u8, alpha* f64, mask u8, F* (H,W,3) f64 in levels, B* likewise)."""
    rng = np.random.default_rng(seed)
    if kind == "strands":
        img, a, m = strand_scene(h, w, seed=seed)
        for _ in range(12):
            rng.uniform(0.2, 0.8)
    elif kind == "disk":
        img, a, m = soft_disk_scene(h, w, 40.0, 3.0, seed)
    else:
        raise ValueError(kind)
    fg, bg = _smooth_texture(rng, h, w, 150, 250), _smooth_texture(rng, h, w, 10, 110)
    assert np.array_equal(img, np.rint(a[..., None] * fg + (1.0 - a[..., None]) * bg).astype(np.uint8))
    return img, a, m, fg, bg


def to_u8(x) -> np.ndarray:
    return np.floor(255.0 * np.clip(x, 0.0, 1.0) + 0.5).astype(np.uint8)


def premult_error(a, colour, alpha_true, f_true, region) -> float:
    """sum over the region and channels of |a C - alpha* F* / 255|."""
    return float(np.abs(a[..., None] * colour - alpha_true[..., None] * f_true / 255.0)[region].sum())


ALPHA_SOURCES = ("true", "closed", "guided")


def alpha_input(kind: str, seed: int, source: str) -> np.ndarray:
    """The float32 alpha the quality and agreement tests feed the solver, from the restatements alone: the true alpha,
    the closed-form matte at its defaults clipped to [0, 1], or the guided matte with radius 4, eps 1e-4."""
    from closed_form_ref import pcg as closed_form_pcg
    from matte_ref import alpha_matte_ref
    img, a_true, mask, _, _ = scene_colours(kind, seed)
    if source == "true":
        a = a_true
    elif source == "closed":
        a = np.clip(closed_form_pcg(img, mask, 1, 1e-5, 1, 500, 1e-4)[0], 0.0, 1.0)
    elif source == "guided":
        a = alpha_matte_ref(img, mask, 4, 1e-4)
    else:
        raise ValueError(source)
    return np.asarray(a, np.float64).astype(np.float32)


def quality_ratio(alpha, F, bgr, alpha_true, f_true, region) -> float:
    """error(alpha', clamp(F)) / error(alpha, I): the premultiplied colour error of the clean cut-out over that of the
    cut-out that keeps the image's bytes (alpha the solver's input, unsnapped, for the latter)."""
    a = np.asarray(alpha, np.float64)
    clean = premult_error(snap(a), np.clip(F, 0.0, 1.0), alpha_true, f_true, region)
    return clean / premult_error(a, np.asarray(bgr, np.float64) / 255.0, alpha_true, f_true, region)


def premult_levels(alpha_snapped, F, B):
    """(alpha' clamp(F), (1 - alpha') clamp(B)) in byte levels: what the agreement test compares."""
    a = np.asarray(alpha_snapped, np.float64)[..., None]
    return 255.0 * a * np.clip(F, 0.0, 1.0), 255.0 * (1.0 - a) * np.clip(B, 0.0, 1.0)
