"""The exact distance transform of a mask and its modifiers (include/ggc.h K2, K3) restated in plain numpy integers, from
the header's text and not from the kernels.

Pixels (y, x) and (y', x') are d2 = (y-y')^2 + (x-x')^2 apart.  A background pixel carries +min d2 to a foreground pixel, a
foreground pixel -min d2 to a background pixel; where no opposite pixel exists the magnitude is FAR.  With
border_background every position outside the image is background, realised here by padding the mask with a background ring
of width max(H, W) and cropping (the kernels use a closed form instead).  A cap reports every magnitude above it as FAR.
The modifiers are explicit disk dilations and erosions, not thresholds of the transform, so the two definitions check each
other (tests/test_distance_ref_cpu.py)."""
import numpy as np

FAR = 2 ** 31 - 1
BORDER_BG = 1
GROW, SHRINK, BORDER, OPEN, CLOSE, TRIMAP = range(6)
_NONE = np.int64(1) << 40        # a flag, never a number: it is replaced before any sum is read


def _d2_to(sites, r0, r1, c0, c1):
    """min d2 from every pixel of rows r0..r1, columns c0..c1 to the set pixels of `sites`; FAR where there is none."""
    hs, ws = sites.shape
    ys = np.arange(hs, dtype=np.int64)[:, None]
    xs = np.arange(ws, dtype=np.int64)[None, :]
    cols = np.arange(c0, c1, dtype=np.int64)[:, None]
    out = np.full((r1 - r0, c1 - c0), FAR, np.int64)
    for y in range(r0, r1):
        g = np.min(np.broadcast_to(np.abs(ys - y), sites.shape), axis=0, where=sites, initial=_NONE)    # column distances of this row
        have = g < _NONE
        if not have.any():
            continue
        g2 = np.where(have, g, 0) ** 2
        table = np.where(have[None, :], g2[None, :] + (xs - cols) ** 2, FAR)        # [c1 - c0, ws]
        out[y - r0] = table.min(axis=1)
    return out


def signed_d2(mask, border_background=False, max_dist2=0):
    """(H, W) mask, any nonzero value foreground -> (H, W) int32."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    p = max(h, w) if border_background else 0
    padded = np.pad(m, p)                                               # a ring of background
    d_out = _d2_to(padded, p, p + h, p, p + w)
    d_in = _d2_to(~padded, p, p + h, p, p + w)
    return apply_cap(np.where(m, -d_in, d_out).astype(np.int32), max_dist2)


def signed_d2_window(mask, r0, r1, c0, c1, border_background=False, max_dist2=0):
    """signed_d2(mask)[r0:r1, c0:c1] without computing the rest: for the shapes at the size limit."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    p = max(h, w) if border_background else 0
    padded = np.pad(m, p)
    d_out = _d2_to(padded, p + r0, p + r1, p + c0, p + c1)
    d_in = _d2_to(~padded, p + r0, p + r1, p + c0, p + c1)
    return apply_cap(np.where(m[r0:r1, c0:c1], -d_in, d_out).astype(np.int32), max_dist2)


def apply_cap(signed, max_dist2):
    """The cap of K2 on an unbounded result: every magnitude above max_dist2 > 0 becomes FAR, the sign stays."""
    d = np.asarray(signed).astype(np.int64)
    if max_dist2 > 0:
        d = np.where(np.abs(d) > max_dist2, np.sign(d) * FAR, d)
    return d.astype(np.int32)


def signed_d2_brute(mask, border_background=False, max_dist2=0):
    """The same by a loop over all pixel pairs (shapes up to 12 x 12)."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    assert h <= 12 and w <= 12
    p = max(h, w) if border_background else 0
    out = np.zeros((h, w), np.int32)
    for y in range(h):
        for x in range(w):
            best = FAR
            for yy in range(-p, h + p):
                for xx in range(-p, w + p):
                    other = bool(m[yy, xx]) if (0 <= yy < h and 0 <= xx < w) else False
                    if other != bool(m[y, x]):
                        best = min(best, (y - yy) ** 2 + (x - xx) ** 2)
            if max_dist2 > 0 and best > max_dist2:
                best = FAR
            out[y, x] = -best if m[y, x] else best
    return out


def signed_d2_batch(masks, border_background=False, max_dist2=0):
    return np.stack([signed_d2(m, border_background, max_dist2) for m in masks])


def _offsets(r2):
    r = int(np.floor(np.sqrt(r2)))
    while (r + 1) ** 2 <= r2:
        r += 1
    while r * r > r2:
        r -= 1
    return r, [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= r2]


def grow(mask, r2):
    """Dilation by the disk dy^2 + dx^2 <= r2: any over the offsets; nothing is foreground outside the image."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    r, offs = _offsets(r2)
    pad = np.pad(m, r)
    out = np.zeros((h, w), bool)
    for dy, dx in offs:
        out |= pad[r + dy:r + dy + h, r + dx:r + dx + w]
    return out.astype(np.uint8)


def shrink(mask, r2, border_background=False):
    """Erosion by the same disk: all over the offsets; outside the image is background with the flag, absent without."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    r, offs = _offsets(r2)
    pad = np.pad(m, r, constant_values=not border_background)
    out = np.ones((h, w), bool)
    for dy, dx in offs:
        out &= pad[r + dy:r + dy + h, r + dx:r + dx + w]
    return out.astype(np.uint8)


def modify(mask, op, r2_a, r2_b=0, border_background=False):
    """One op of ggc_modify_mask on an (H, W) mask -> uint8."""
    if op == GROW:
        return grow(mask, r2_a)
    if op == SHRINK:
        return shrink(mask, r2_a, border_background)
    if op == BORDER:
        return (grow(mask, r2_b) & (1 - shrink(mask, r2_a, border_background))).astype(np.uint8)
    if op == OPEN:
        return grow(shrink(mask, r2_a, border_background), r2_a)
    if op == CLOSE:
        return shrink(grow(mask, r2_a), r2_a, border_background)
    if op == TRIMAP:
        inner, outer = shrink(mask, r2_a, border_background), grow(mask, r2_b)
        return np.where(inner != 0, 255, np.where(outer != 0, 128, 0)).astype(np.uint8)
    raise ValueError(op)


def modify_batch(masks, op, r2_a, r2_b=0, border_background=False):
    return np.stack([modify(m, op, r2_a, r2_b, border_background) for m in masks])
