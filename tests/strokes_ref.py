"""Brush strokes in plain Python integers, written from the contract of ggc_apply_strokes / ggc_stroke_pixels in
include/ggc.h (H2), not from the kernel.  NumPy only carries arrays of Python ints (dtype=object), so no product can
overflow: the rule needs up to 90 bits."""
import numpy as np


def segments_of(fg_strokes, bg_strokes):
    """Polylines -> [(r0, c0, r1, c1, label)]: foreground strokes first, then background; a polyline of n >= 2 vertices is
    its n-1 segments, a one-vertex stroke one segment with both ends equal."""
    out = []
    for label, strokes in ((1, fg_strokes or ()), (0, bg_strokes or ())):
        for stroke in strokes:
            v = [(int(r), int(c)) for r, c in stroke]
            assert v, "empty stroke"
            pairs = [(v[0], v[0])] if len(v) == 1 else list(zip(v[:-1], v[1:]))
            out += [(a[0], a[1], b[0], b[1], label) for a, b in pairs]
    return out


def within(h, w, seg, radius):
    """(h, w) bool: the pixels within rho of the segment, 4 dist^2 <= rho4 = max(4 radius^2, 1)."""
    r0, c0, r1, c1 = (int(v) for v in seg[:4])
    rho4 = max(4 * int(radius) * int(radius), 1)
    yy, xx = np.mgrid[0:h, 0:w]
    wy, wx = yy.astype(object) - r0, xx.astype(object) - c0
    dy, dx = r1 - r0, c1 - c0
    l2 = dy * dy + dx * dx
    t = wy * dy + wx * dx
    ey, ex = wy - dy, wx - dx
    cr = wy * dx - wx * dy
    head = (4 * (wy * wy + wx * wx) <= rho4).astype(bool)
    tail = (4 * (ey * ey + ex * ex) <= rho4).astype(bool)
    mid = (4 * cr * cr <= rho4 * l2).astype(bool)
    return np.where((t <= 0).astype(bool), head, np.where((t >= l2).astype(bool), tail, mid))


def labels(h, w, segs, radius):
    """(h, w) int: the label the image's segments paint at each pixel, the last segment winning; -1 where none does."""
    lab = np.full((h, w), -1, np.int32)
    for seg in segs:
        lab[within(h, w, seg, radius)] = 1 if seg[4] != 0 else 0
    return lab


def paint(mask, segs, radius):
    out = np.array(mask, dtype=np.uint8, copy=True)
    lab = labels(*out.shape, segs, radius)
    out[lab >= 0] = lab[lab >= 0]
    return out


def pixels(h, w, segs):
    """(P, 3) int32 = (row, col, label): the centre-line pixels (radius 0) inside the image, in raster order."""
    lab = labels(h, w, segs, 0)
    r, c = np.nonzero(lab >= 0)                       # np.nonzero walks in raster order
    return np.stack([r, c, lab[r, c]], 1).astype(np.int32).reshape(-1, 3)


def pack(per_image):
    """[list of segments per image] -> (strokes int32 [S,5], stroke_ptr int32 [B+1])."""
    rows = [s for segs in per_image for s in segs]
    ptr = np.concatenate([[0], np.cumsum([len(segs) for segs in per_image])]).astype(np.int32)
    return np.asarray(rows, np.int32).reshape(-1, 5), ptr


# ((h, w), segment, radius): long segments through small images.  The first six are the cases named when the entries were
# specified; on a 20x30 image their products still fit 64 bits, so the last three are added, where a signed 64-bit
# compare provably goes wrong (rho4 L2 >= 2^63 at the largest radius; (w x d)^2 >= 2^61 far from a steep line).
LONG_CASES = [
    ((20, 30), (-30000, -30000, 30020, 30030, 1), 0),
    ((20, 30), (-30000, -30000, 30020, 30030, 1), 3),
    ((20, 30), (-2**20, -2**20, 2**20, 2**20 - 7, 1), 0),
    ((20, 30), (-2**20, -2**20, 2**20, 2**20 - 7, 1), 3),
    ((20, 30), (2**20, -2**20, -2**20, 2**20, 0), 0),
    ((20, 30), (2**20, -2**20, -2**20, 2**20, 0), 3),
    ((20, 30), (-2**20, -2**20, 2**20, 2**20 - 7, 1), 16384),
    ((3, 2000), (-2**20, 2**20, 2**20, -2**20 + 40, 1), 0),
    ((3, 2000), (-2**20, 2**20, 2**20, -2**20 + 40, 1), 3),
]
LONG_CASES_BEYOND_64_BITS = (6, 7, 8)
