"""A float64 GrabCut written from the specification, and the step certificate that judges the device and the oracle by it.

cv2.grabCut is not available, and oracle/grabcut.c is this project's own restatement of it, so an error the two share
passes every parity test.  This module restates one GrabCut iteration from SURVEY.md Appendix A.4 and the reference's
grabcut.py:81-168 in vectorised numpy with libm exp / log (np.exp, np.log).  It uses the oracle only as a max-flow
solver (oracle.grid_maxflow, pinned against scipy in tests/test_grabcut_oracle.py).

One iteration, given the previous mask and models (cv2 semantics):
  assign   each pixel takes the first component of its class's GMM with the strictly largest linear score
           coef > 0 ? det^-1/2 exp(-mahal/2) : 0 (component 0 when every score is 0)
  learn    per class and component from int64 sums: coef n/total, mean, cov = E[xx^T] - mu mu^T, +0.01 on the diagonal
           when det <= 1e-6; an empty component gets coef 0 and keeps its previous mean and cov
  t-links  probable pixels: (-log p_bg, -log p_fg) with p = sum_ci coef * score; BGD (0, lambda), FGD (lambda, 0)
  n-links  gamma exp(-beta |dI|^2), / sqrt(2) on the diagonals; beta = 1 / (2 sum / (4WH - 3W - 3H + 2)), 0 if sum = 0

and the project's documented deviations, each a named step: cancel_clamp (source minus sink,
clamped to +-lambda), nan_to_zero (inf - inf when both totals are 0), quantise (rint at scale 2^18).

flush_below emulates exp(x) = 0 for x < flush_below and log(subnormal) = -inf, the behaviour of the deterministic
exp / log before they were extended to the subnormal range; the underflow families use it to prove they reach it.

Families (make()) aim at one mechanism each.  A start state is (img, mask, mode, rect, bgd, fgd): mode 2 starts carry
hand-made models, mode 0 / 1 starts get their k-means models from the call with n_iter = 0.
"""
import math

import numpy as np

GC_BGD, GC_FGD, GC_PR_BGD, GC_PR_FGD = 0, 1, 2, 3
NCOMP = 5
GAMMA = 50.0
LAMBDA = 9.0 * GAMMA
SCALE = float(1 << 18)
PLANE_OFF = [(0, -1), (-1, -1), (-1, 0), (-1, 1)]   # left, up-left, up, up-right: the oracle's n-link planes
AMBIG_TOL = 1e-6
TIE_REL = 1e-12


# ------------------------------------------------------------------ mask set-up (grabcut.py:81-151)

def init_rect(h, w, rect):
    """GC_INIT_WITH_RECT: outside 0, inside 3.  Negative x / y shorten the width / height (the project's rule; whether
    OpenCV 4.x clamps without shortening is unverified)."""
    x, y, rw, rh = (int(v) for v in rect)
    if x < 0:
        rw, x = rw + x, 0
    if y < 0:
        rh, y = rh + y, 0
    rw, rh = min(rw, w - x), min(rh, h - y)
    m = np.zeros((h, w), np.uint8)
    if rw > 0 and rh > 0:
        m[y:y + rh, x:x + rw] = GC_PR_FGD
    return m


def init_trimap(trimap):
    """run_with_trimap: promote probable labels when a definite class is missing; -> (mask, degenerate)."""
    t = np.array(trimap, np.uint8)
    if not (t == GC_FGD).any():
        t[t == GC_PR_FGD] = GC_FGD
    if not (t == GC_BGD).any():
        t[t == GC_PR_BGD] = GC_BGD
    return t, not ((t == GC_FGD).any() and (t == GC_BGD).any())


def probable(mask):
    return (mask == GC_PR_BGD) | (mask == GC_PR_FGD)


def is_fg(mask):
    return (mask == GC_FGD) | (mask == GC_PR_FGD)


# ------------------------------------------------------------------ beta and n-links

def _pairs(img):
    """(plane, |dI|^2 (H,W) int64 with 0 outside, in-image (H,W) bool) for the four half-neighbour directions."""
    h, w = img.shape[:2]
    a = img.astype(np.int64)
    out = []
    for k, (dy, dx) in enumerate(PLANE_OFF):
        d2 = np.zeros((h, w), np.int64)
        ok = np.zeros((h, w), bool)
        ys, xs = slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx))
        yq, xq = slice(max(0, -dy) + dy, h - max(0, dy) + dy), slice(max(0, -dx) + dx, w - max(0, dx) + dx)
        d2[ys, xs] = ((a[ys, xs] - a[yq, xq]) ** 2).sum(-1)
        ok[ys, xs] = True
        out.append((k, d2, ok))
    return out


def beta(img):
    h, w = img.shape[:2]
    s = sum(int(d2.sum()) for _, d2, _ in _pairs(img))
    return 0.0 if s == 0 else 1.0 / (2.0 * s / (4 * w * h - 3 * w - 3 * h + 2))


def nlinks(img):
    """(4, H, W) float64 n-link weights in the oracle's plane layout, 0 where the neighbour is outside."""
    b = beta(img)
    h, w = img.shape[:2]
    nw = np.zeros((4, h, w))
    for k, d2, ok in _pairs(img):
        wt = GAMMA * np.exp(-b * d2.astype(np.float64))
        if k & 1:
            wt = wt / math.sqrt(2.0)
        nw[k] = np.where(ok, wt, 0.0)
    return nw


# ------------------------------------------------------------------ GMMs

def unpack(model):
    m = np.asarray(model, np.float64).ravel()
    return m[:5].copy(), m[5:20].reshape(5, 3).copy(), m[20:65].reshape(5, 3, 3).copy()


def pack(coef, mean, cov):
    return np.concatenate([coef, mean.ravel(), cov.ravel()])


def _exp(x, flush_below):
    with np.errstate(under="ignore", over="ignore"):
        e = np.exp(x)
    return e if flush_below is None else np.where(x < flush_below, 0.0, e)


def _log(x, flush_below):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.log(x)
    return r if flush_below is None else np.where(x < np.finfo(np.float64).tiny, -np.inf, r)


def scores(model, px, flush_below=None):
    """(P, 5) linear component scores coef > 0 ? det^-1/2 exp(-mahal/2) : 0 of colours px (P, 3), and the exponents."""
    coef, mean, cov = unpack(model)
    s = np.zeros((len(px), NCOMP))
    ex = np.full((len(px), NCOMP), -np.inf)
    for ci in range(NCOMP):
        if not coef[ci] > 0.0:
            continue
        d = px.astype(np.float64) - mean[ci]
        mahal = np.einsum("pi,ij,pj->p", d, np.linalg.inv(cov[ci]), d)
        ex[:, ci] = -0.5 * mahal
        s[:, ci] = np.linalg.det(cov[ci]) ** -0.5 * _exp(-0.5 * mahal, flush_below)
    return s, ex


def total(model, px, flush_below=None):
    coef = unpack(model)[0]
    return (scores(model, px, flush_below)[0] * coef).sum(1)


def assign(img, mask, bgd, fgd, flush_below=None):
    """assignGMMsComponents -> (comp (H,W) int, near_tie (H,W) bool)."""
    px = img.reshape(-1, 3)
    fg = is_fg(mask).ravel()
    comp = np.zeros(px.shape[0], np.int64)
    tie = np.zeros(px.shape[0], bool)
    for cls, model in ((False, bgd), (True, fgd)):
        sel = fg == cls
        s, _ = scores(model, px[sel], flush_below)
        comp[sel] = np.argmax(s, 1)                 # first maximum; all-zero rows give 0
        top = np.sort(s, 1)
        tie[sel] = (top[:, -1] > 0) & (top[:, -1] - top[:, -2] <= TIE_REL * top[:, -1])
    return comp.reshape(mask.shape), tie.reshape(mask.shape)


def learn(img, mask, comp, bgd_prev, fgd_prev):
    """learnGMMs from int64 sums -> (bgd, fgd) 65-vectors."""
    px = img.reshape(-1, 3).astype(np.int64)
    fg = is_fg(mask).ravel()
    c = comp.ravel()
    out = []
    for cls, prev in ((False, bgd_prev), (True, fgd_prev)):
        coef, mean, cov = unpack(prev)
        sel = fg == cls
        n_tot = int(sel.sum())
        for ci in range(NCOMP):
            x = px[sel & (c == ci)]
            n = len(x)
            if n == 0:
                coef[ci] = 0.0
                continue
            s1 = x.sum(0)
            s2 = x.T @ x                            # exact: at most 2^16 * P
            coef[ci] = n / n_tot
            mean[ci] = s1 / n
            cv = s2 / n - np.outer(mean[ci], mean[ci])
            if np.linalg.det(cv) <= 1e-6:
                cv = cv + 0.01 * np.eye(3)
            cov[ci] = cv
        out.append(pack(coef, mean, cov))
    return out[0], out[1]


# ------------------------------------------------------------------ t-links and the documented deviations

def tlinks(img, mask, bgd, fgd, flush_below=None):
    """(from_source, to_sink) float64 (H,W): -log totals for probable pixels, (0, lambda) / (lambda, 0) for BGD / FGD."""
    px = img.reshape(-1, 3)
    src = -_log(total(bgd, px, flush_below), flush_below).reshape(mask.shape)
    snk = -_log(total(fgd, px, flush_below), flush_below).reshape(mask.shape)
    src = np.where(mask == GC_BGD, 0.0, np.where(mask == GC_FGD, LAMBDA, src))
    snk = np.where(mask == GC_BGD, LAMBDA, np.where(mask == GC_FGD, 0.0, snk))
    return src, snk


def cancel_clamp(src, snk):
    """Deviation 2a: one signed t-link per pixel, source minus sink, clamped to +-lambda (no cut changes)."""
    with np.errstate(invalid="ignore"):
        return np.clip(src - snk, -LAMBDA, LAMBDA)


def nan_to_zero(d):
    """Deviation 2b: inf - inf (both totals exactly 0, where cv2's capacities would be NaN) becomes 0."""
    return np.where(np.isnan(d), 0.0, d)


def quantise(w):
    """Deviation 2c: int32 capacities at scale 2^18, rounded half to even."""
    return np.rint(w * SCALE).astype(np.int32)


def network(img, mask, bgd, fgd, flush_below=None):
    """-> (tw (H,W) int32, nw (4,H,W) int32, twf, nwf float64): the quantised network in grid_maxflow's layout and
    its unquantised float64 capacities."""
    twf = nan_to_zero(cancel_clamp(*tlinks(img, mask, bgd, fgd, flush_below)))
    nwf = nlinks(img)
    return quantise(twf), quantise(nwf), twf, nwf


def ambiguous(twf, nwf, tol=AMBIG_TOL):
    """Capacities whose scaled value lies within tol of a half-integer: another last ulp may round them the other way."""
    n = 0
    for a in (twf, nwf):
        s = np.abs(a * SCALE)
        n += int((np.abs(s - np.floor(s) - 0.5) <= tol).sum())
    return n


def _cut_links(fg, nw):
    """(4, H, W) bool: the link of the plane crosses the cut."""
    h, w = fg.shape
    out = np.zeros((4, h, w), bool)
    for k, (dy, dx) in enumerate(PLANE_OFF):
        ys, xs = slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx))
        yq, xq = slice(max(0, -dy) + dy, h - max(0, dy) + dy), slice(max(0, -dx) + dx, w - max(0, dx) + dx)
        out[k, ys, xs] = fg[ys, xs] != fg[yq, xq]
    return out


def energy64(fg, twf, nwf):
    """GrabCut energy of the labelling fg (H,W) bool on the unquantised network: a pixel on the source (foreground)
    side pays its sink link, one on the sink side its source link, plus every n-link that crosses the cut."""
    data = np.where(fg, np.maximum(-twf, 0.0), np.maximum(twf, 0.0)).sum()
    return float(data + nwf[_cut_links(fg, nwf)].sum())


def cut_capacity(fg, tw, nw):
    """The same on the quantised network, exact in int64."""
    tw = tw.astype(np.int64)
    data = np.where(fg, np.maximum(-tw, 0), np.maximum(tw, 0)).sum()
    return int(data + nw.astype(np.int64)[_cut_links(fg, nw)].sum())


def n_links(h, w):
    return 4 * h * w - 3 * w - 3 * h + 2


def step(img, mask, bgd, fgd, flush_below=None):
    """One iteration from (mask, models): -> dict comp, tie, bgd, fgd, tw, nw, twf, nwf."""
    comp, tie = assign(img, mask, bgd, fgd, flush_below)
    nb, nf = learn(img, mask, comp, bgd, fgd)
    tw, nw, twf, nwf = network(img, mask, nb, nf, flush_below)
    return dict(comp=comp, tie=tie, bgd=nb, fgd=nf, tw=tw, nw=nw, twf=twf, nwf=nwf)


def band_pixels(img, mask, bgd, fgd, lo=-745.2, hi=-708.0):
    """Probable pixels for which, under one of the two GMMs, the largest component exponent lies in (lo, hi)."""
    px = img.reshape(-1, 3)
    pr = probable(mask).ravel()
    hit = np.zeros(len(px), bool)
    for model in (bgd, fgd):
        mx = scores(model, px)[1].max(1)
        hit |= (mx > lo) & (mx < hi)
    return (hit & pr).reshape(mask.shape)


# ------------------------------------------------------------------ the certificate of one iteration

def _models_close(got, want, what):
    gc, gm, gv = unpack(got)
    wc, wm, wv = unpack(want)
    np.testing.assert_allclose(gc, wc, rtol=1e-12, atol=0, err_msg=f"{what}: coefs")
    live = wc > 0
    np.testing.assert_allclose(gm[live], wm[live], rtol=1e-12, atol=1e-12, err_msg=f"{what}: means")
    # cov = E[xx^T] - mu mu^T cancels: its rounding error scales with E[xx^T] <= 255^2, not with the covariance
    np.testing.assert_allclose(gv[live], wv[live], rtol=1e-12, atol=1e-12 * 65025, err_msg=f"{what}: covariances")


def certify_step(orc, img, mask0, bgd0, fgd0, mask1, bgd1, fgd1, what="", exact_ties=False):
    """Assert that (bgd1, fgd1, mask1) is a correct GrabCut iteration from (mask0, bgd0, fgd0).

    * definite pixels keep their label, probable pixels stay probable;
    * with no near-tie assignment (or only exact ties, which both sides must break to the lowest index), the models
      equal learn(assign(models0)) to rtol 1e-12;
    * with no ambiguous capacity, the probable pixels equal the canonical cut of the reference network; otherwise the
      cut of mask1 exceeds the minimum by at most 2 units per ambiguous capacity;
    * the float64 energy of mask1 is within the quantisation bound of the reference cut's.
    Returns the reference step and the number of ambiguous capacities."""
    img = np.asarray(img)
    h, w = mask0.shape
    ref = step(img, mask0, bgd0, fgd0)
    pr = probable(mask0)
    assert np.array_equal(mask1[~pr], mask0[~pr]), f"{what}: a definite pixel changed"
    assert probable(mask1)[pr].all(), f"{what}: a probable pixel became definite"
    ties = bool(ref["tie"].any())
    if not ties or exact_ties:
        _models_close(bgd1, ref["bgd"], f"{what} background")
        _models_close(fgd1, ref["fgd"], f"{what} foreground")
        tw, nw, twf, nwf = ref["tw"], ref["nw"], ref["twf"], ref["nwf"]
    else:                                            # the assignment is not decidable here: certify the cut on the models
        tw, nw, twf, nwf = network(img, mask0, bgd1, fgd1)
    amb = ambiguous(twf, nwf)
    _, side = orc.grid_maxflow(tw, nw)
    want = side.astype(bool)
    got = is_fg(mask1)
    assert np.array_equal(want[~pr], got[~pr]), f"{what}: the reference cut moved a definite pixel"
    if amb == 0:
        bad = int((want[pr] != got[pr]).sum())
        assert bad == 0, f"{what}: {bad} probable pixels differ from the reference cut"
    else:
        extra = cut_capacity(got, tw, nw) - cut_capacity(want, tw, nw)
        assert extra <= 2 * amb, f"{what}: cut exceeds the minimum by {extra} > 2 * {amb} ambiguous capacities"
    e_got, e_ref = energy64(got, twf, nwf), energy64(want, twf, nwf)
    slack = 2 * (h * w + n_links(h, w)) * 2.0 ** -19
    assert e_got <= e_ref + slack + 1e-12 * abs(e_ref), f"{what}: energy {e_got} > {e_ref} + {slack}"
    return ref, amb


# ------------------------------------------------------------------ adversarial families

def model(comps):
    """65-vector from [(coef, mean(3), cov diag(3) or 3x3)]."""
    coef, mean, cov = np.zeros(5), np.zeros((5, 3)), np.tile(np.eye(3), (5, 1, 1))
    for ci, (c, m, v) in enumerate(comps):
        coef[ci] = c
        mean[ci] = m
        v = np.asarray(v, np.float64)
        cov[ci] = np.diag(v) if v.ndim == 1 else v
    return pack(coef, mean, cov)


def _underflow(rng, variant):
    """Two band pixels of colour C sit in definite background that mixes A and A + (2, 0, 0): the learned background
    component there has variance 1.01 along the first channel, so C = A + (39, 0, 0) has exponent -714.9 under it
    (libm: -log p_bg = 710.4; flushed: +inf).  A checkerboard of A and its complement keeps beta small, so the band
    pixel's eight n-links sum to about 320.  The band pixels share the single foreground component with a flat
    definite-foreground block of n pixels, which puts -log p_fg at about n / 4:
      one_side      n = 1800: -log p_fg = 447, so libm's t-link 263 < 320 loses to the n-links; flushed it is +450
      both_sides    n = 2900: the foreground exponent is in the band too (-725); flushed the t-link is inf - inf -> 0
      assign_flush  n = 1800, and the previous foreground GMM has a second component 38 away from C along the third
                    channel (exponent -722): libm assigns the band pixels to it, the flush to component 0."""
    A = np.array([40, 60, 80])
    Ab = 255 - A
    F = np.array([200, 200, 40])
    C = A + np.array([39, 0, 0])
    h, w = 96, 112
    img = np.zeros((h, w, 3), np.uint8)
    img[:] = A
    img[rng.random((h, w)) < 0.5] = A + np.array([2, 0, 0])
    yy, xx = np.mgrid[:h, :w]
    img[(yy < 16) & ((yy + xx) % 2 == 1)] = Ab
    mask = np.zeros((h, w), np.uint8)
    nf = 2900 if variant == "both_sides" else 1800
    blk = np.zeros(h * w, bool)
    blk[[(36 + i // 50) * w + 4 + i % 50 for i in range(nf)]] = True
    blk = blk.reshape(h, w)
    img[blk] = F
    mask[blk] = GC_FGD
    for y, x in ((20, 70), (28, 90)):
        img[y, x] = C
        mask[y, x] = GC_PR_FGD
    bgd = model([(0.9, A, (4.0, 4.0, 4.0)), (0.1, Ab, (4.0, 4.0, 4.0))])
    if variant == "assign_flush":
        fgd = model([(0.5, F, (1.0, 1.0, 1.0)), (0.5, C + np.array([0, 0, 38]), (1.0, 1.0, 1.0))])
    else:
        fgd = model([(1.0, F, (1.0, 1.0, 1.0))])
    return dict(img=img, mask=mask, mode=2, bgd=bgd, fgd=fgd)


def _blobs(h, w, rng, n_colours=None):
    """A small scene: background colour noise, a foreground ellipse, a trimap with a definite border and core."""
    from gcn_grabcut.synthetic import synthetic_image
    img, gt = synthetic_image(h, w, int(rng.integers(1 << 30)), return_mask=True)
    if n_colours is not None:                        # quantise the foreground to a few distinct colours
        pal = rng.integers(0, 256, (n_colours, 3))
        img[gt == 1] = pal[rng.integers(0, n_colours, int(gt.sum()))]
    return img, gt


def trimap_of(gt, border=3, core=2):
    h, w = gt.shape
    t = np.full((h, w), GC_PR_BGD, np.uint8)
    t[gt == 1] = GC_PR_FGD
    b = min(border, h // 4, w // 4)
    if b > 0:
        t[:b] = GC_BGD; t[-b:] = GC_BGD; t[:, :b] = GC_BGD; t[:, -b:] = GC_BGD
    ys, xs = np.nonzero(gt)
    if len(ys):
        cy, cx = int(ys.mean()), int(xs.mean())
        t[max(0, cy - core):cy + core + 1, max(0, cx - core):cx + core + 1] = GC_FGD
    return t


def _singular(rng, variant):
    h, w = 48, 64
    if variant == "flat":                            # both classes flat: every covariance takes the +0.01 fix
        img = np.zeros((h, w, 3), np.uint8)
        img[:] = (30, 90, 150)
        gt = np.zeros((h, w), np.uint8)
        gt[12:36, 16:48] = 1
        img[gt == 1] = (220, 40, 90)
        img[20:24, 5:9] = (220, 40, 90)              # probable background that looks like the foreground
        return dict(img=img, mask=trimap_of(gt), mode=0)
    if variant == "single_pixel":                    # the foreground class is one pixel: K = 1, a flat component
        img, _ = _blobs(h, w, rng)
        mask = np.zeros((h, w), np.uint8)
        mask[10:30, 10:40] = GC_PR_BGD
        mask[20, 25] = GC_FGD
        return dict(img=img, mask=mask, mode=0)
    img, gt = _blobs(h, w, rng, n_colours=3)          # few_colours: K-means with K = 5 > 3 distinct colours
    return dict(img=img, mask=trimap_of(gt), mode=0)


def _ties(rng, variant):
    """Colours at the midpoint c of two background components with mirrored means c -+ d and equal covariance: their
    scores are equal to the last bit (64 samples each, so every sum and mean is exact); the lowest index must win."""
    h, w = 32, 48
    c = np.array([100, 120, 140])
    d = np.array([6, -4, 2]) if variant == "mirrored" else np.array([0, 0, 9])
    img = np.zeros((h, w, 3), np.uint8)
    img[:] = c
    mask = np.full((h, w), GC_PR_BGD, np.uint8)
    idx = rng.permutation(h * 16)[:128]
    lo, hi = idx[:64], idx[64:]
    for sel, col in ((lo, c - d), (hi, c + d)):
        img.reshape(-1, 3)[sel] = col
        mask.ravel()[sel] = GC_BGD
    img[:, 32:] = (230, 30, 30)
    mask[:, 32:] = GC_PR_FGD
    mask[10:20, 38:42] = GC_FGD
    cov = np.array([[9.0, 1.0, 0.5], [1.0, 7.0, 0.25], [0.5, 0.25, 5.0]])
    bgd = model([(0.5, c - d, cov), (0.5, c + d, cov)])
    fgd = model([(1.0, (230, 30, 30), (2.0, 2.0, 2.0))])
    return dict(img=img, mask=mask, mode=2, bgd=bgd, fgd=fgd, exact_ties=True)


def _beta(rng, variant):
    h, w = 40, 56
    gt = np.zeros((h, w), np.uint8)
    gt[10:30, 14:42] = 1
    if variant == "zero_contrast":                   # one colour: the beta sum is 0, beta = 0, every n-link is gamma
        img = np.full((h, w, 3), 128, np.uint8)
    else:                                            # max_contrast: a 0 / 255 checkerboard, beta = 1 / 2 / 3 * 255^2 ...
        yy, xx = np.mgrid[:h, :w]
        img = np.repeat(((yy + xx) % 2 * 255).astype(np.uint8)[..., None], 3, -1)
        img[gt == 1] = np.where(((yy + xx) % 2 == 1)[gt == 1, None], 255, 60)
    return dict(img=img, mask=trimap_of(gt), mode=0)


def _shapes(rng, variant):
    """1x1, 1xN, Nx1 and 2x2 images from hand-made models (mode 2 needs no definite pixel)."""
    h, w = {"1x1": (1, 1), "1xN": (1, 97), "Nx1": (83, 1), "2x2": (2, 2)}[variant]
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    mask = rng.integers(0, 4, (h, w)).astype(np.uint8)
    if variant == "1x1":
        mask[:] = GC_PR_FGD
    bgd = model([(0.6, (60, 60, 60), (900.0, 700.0, 800.0)), (0.4, (200, 80, 30), (400.0, 500.0, 300.0))])
    fgd = model([(1.0, (150, 170, 190), (600.0, 600.0, 600.0))])
    return dict(img=img, mask=mask, mode=2, bgd=bgd, fgd=fgd)


def _near_lambda(rng, variant):
    """Probable pixels whose signed t-link sits a few units inside and outside +-lambda.  Definite background and
    foreground are noisy A and F; single-component models make each class one Gaussian.  The probable colours are
    picked from a sweep along A..F by their t-link under the models they are learned with (four re-picks reach the
    fixed point; twelve pixels among 4096 move the models by a few units of t-link)."""
    h, w = 64, 64
    A, F = np.array([50, 80, 110]), np.array([170, 140, 60])
    img = np.zeros((h, w, 3), np.uint8)
    img[:] = A + rng.integers(-7, 8, (h, w, 3))         # variance 18.7: |F - A|^2 / (2 var) = 548 > lambda, and
    img[:, 32:] = F + rng.integers(-7, 8, (h, 32, 3))   # the likelihoods stay normal where the t-link is +-lambda
    mask = np.zeros((h, w), np.uint8)
    mask[:, 32:] = GC_FGD
    bgd = model([(1.0, A, (18.0, 18.0, 18.0))])
    fgd = model([(1.0, F, (18.0, 18.0, 18.0))])
    t = np.linspace(0.0, 1.0, 241)[:, None, None]
    o = np.arange(-4, 5)
    off = np.stack(np.meshgrid(o, o, o), -1).reshape(1, -1, 3)
    cand = np.clip(np.rint(A + t * (F - A) + off), 0, 255).reshape(-1, 3).astype(np.uint8)
    spots = [(8 + 4 * (i % 12), 8 + 16 * (i // 12)) for i in range(12)]
    for _ in range(4):                  # the picks move the learned models a little: re-pick on the new models
        nb, nf = learn(img, mask, np.zeros((h, w), np.int64), bgd, fgd)
        with np.errstate(divide="ignore"):
            d = np.log(total(nf, cand)) - np.log(total(nb, cand))
        picks = []
        for lo, hi in ((-457, -453), (-447, -443), (443, 447), (453, 457)):
            picks += list(rng.choice(np.flatnonzero((d > lo) & (d < hi)), 3, replace=False))
        for (y, x), ci in zip(spots, picks):
            img[y, x] = cand[ci]
            mask[y, x] = GC_PR_FGD if d[ci] > 0 else GC_PR_BGD
    return dict(img=img, mask=mask, mode=2, bgd=bgd, fgd=fgd)


def _rect(rng, variant):
    from gcn_grabcut.synthetic import synthetic_image
    h, w = 60, 80
    img = synthetic_image(h, w, int(rng.integers(1 << 30)))
    rect = {"inside": (10, 8, 50, 40), "touch": (0, 0, 60, 60), "leave": (40, 30, 100, 100),
            "negative": (-10, -5, 40, 30)}[variant]
    return dict(img=img, mask=None, mode=1, rect=rect)


def _colour(rng, variant):
    from oracle import oracle as orc
    img, gt = _blobs(72, 96, rng)
    return dict(img=orc.convert_color8(img, variant), mask=trimap_of(gt), mode=0)


FAMILIES = {
    "underflow": (_underflow, ["one_side", "both_sides", "assign_flush"]),
    "singular": (_singular, ["flat", "single_pixel", "few_colours"]),
    "ties": (_ties, ["mirrored", "axis"]),
    "beta": (_beta, ["zero_contrast", "max_contrast"]),
    "shapes": (_shapes, ["1x1", "1xN", "Nx1", "2x2"]),
    "near_lambda": (_near_lambda, ["sweep"]),
    "rect": (_rect, ["inside", "touch", "leave", "negative"]),
    "colour": (_colour, ["hsv", "lab"]),
}


def make(family, variant, seed=0):
    """A start state: dict img, mask (None in rect mode), mode, and rect or bgd / fgd, exact_ties."""
    fn, variants = FAMILIES[family]
    assert variant in variants, (family, variant)
    st = fn(np.random.default_rng(seed), variant)
    st.setdefault("rect", None)
    st.setdefault("exact_ties", False)
    return st


def cases():
    return [(f, v) for f, (_, vs) in FAMILIES.items() for v in vs]


def start(orc, st, seed=0):
    """(mask0, bgd0, fgd0): the state before iteration 1, through the oracle's call with n_iter = 0 in modes 0 / 1
    (set-up and k-means) and as given in mode 2.  rc 1 (degenerate trimap) returns None."""
    if st["mode"] == 2:
        return st["mask"].copy(), st["bgd"].copy(), st["fgd"].copy()
    _, m, b, f, rc = orc.grabcut(st["img"], st["mask"], n_iter=0, mode=st["mode"], rect=st["rect"], seed=seed)
    if rc:
        return None
    h, w = st["img"].shape[:2]
    want = init_rect(h, w, st["rect"]) if st["mode"] == 1 else init_trimap(st["mask"])[0]
    assert np.array_equal(m, want), "mask set-up differs from the reference"
    return m, b, f
