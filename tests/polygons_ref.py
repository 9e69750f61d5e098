"""The polygon rule of include/ggc.h (H3) restated in Python integers, from the header's text and not from the kernel.

A polygon is n >= 3 integer vertices (row, col), closed implicitly from the last to the first.  Pixel p = (r, c) is COVERED
iff (a) it lies on an edge a -> b: (b.r - a.r)(c - a.c) - (b.c - a.c)(r - a.r) == 0 inside the edge's bounding box, or (b)
its crossing number is odd: an edge counts iff (a.r <= r) != (b.r <= r) and, with lo / hi its ends ordered by row,
(hi.c - lo.c)(r - lo.r) - (c - lo.c)(hi.r - lo.r) > 0.  Python integers do not overflow, so nothing here depends on a
word size."""
import numpy as np

BGD, FGD = 0, 1
BG_FILL, FG_FILL, LASSO = 0, 1, 2


def covered_pixel(r, c, polygon):
    r, c = int(r), int(c)
    n = len(polygon)
    crossings = 0
    for i in range(n):
        ar, ac = (int(v) for v in polygon[i])
        br, bc = (int(v) for v in polygon[(i + 1) % n])
        if (br - ar) * (c - ac) - (bc - ac) * (r - ar) == 0 and min(ar, br) <= r <= max(ar, br) and min(ac, bc) <= c <= max(ac, bc):
            return True
        if (ar <= r) != (br <= r):
            (lr, lc), (hr, hc) = ((ar, ac), (br, bc)) if ar < br else ((br, bc), (ar, ac))
            if (hc - lc) * (r - lr) - (c - lc) * (hr - lr) > 0:
                crossings += 1
    return crossings % 2 == 1


def covered(shape, polygon, origin=(0, 0)):
    """(H, W) bool: the covered pixels of the window whose top-left pixel is `origin`."""
    h, w = shape
    out = np.zeros((h, w), bool)
    for r in range(h):
        for c in range(w):
            out[r, c] = covered_pixel(r + origin[0], c + origin[1], polygon)
    return out


def covered_np(shape, polygon, origin=(0, 0)):
    """covered() for the larger windows of the device tests: the same rule, all pixels at once in numpy int64 (every product
    stays below 2^44 under the header's limits; tests/test_polygons_cpu.py holds it against covered())."""
    h, w = shape
    r = (np.arange(h, dtype=np.int64) + int(origin[0]))[:, None]
    c = (np.arange(w, dtype=np.int64) + int(origin[1]))[None, :]
    on = np.zeros((h, w), bool)
    odd = np.zeros((h, w), bool)
    n = len(polygon)
    for i in range(n):
        ar, ac = (int(v) for v in polygon[i])
        br, bc = (int(v) for v in polygon[(i + 1) % n])
        on |= ((br - ar) * (c - ac) - (bc - ac) * (r - ar) == 0) & (min(ar, br) <= r) & (r <= max(ar, br)) \
            & (min(ac, bc) <= c) & (c <= max(ac, bc))
        (lr, lc), (hr, hc) = ((ar, ac), (br, bc)) if ar < br else ((br, bc), (ar, ac))
        odd ^= ((ar <= r) != (br <= r)) & ((hc - lc) * (r - lr) - (c - lc) * (hr - lr) > 0)
    return on | odd


def apply(mask, polygons, covered=covered):
    """One image: mask (H, W) uint8, polygons = [(label, vertices), ...] in polygon order -> the painted copy.  Lassos
    first (outside all of them: BGD), then the fills in order."""
    out = np.array(mask, np.uint8, copy=True)
    lassos = [v for l, v in polygons if l == LASSO]
    if lassos:
        inside = np.zeros(out.shape, bool)
        for v in lassos:
            inside |= covered(out.shape, v)
        out[~inside] = BGD
    for l, v in polygons:
        if l != LASSO:
            out[covered(out.shape, v)] = FGD if l == FG_FILL else BGD
    return out


def apply_packed(mask, verts, poly_ptr, poly_label, image_ptr, covered=covered_np):
    """The batch call on ggc_apply_polygons' four arrays: mask (B, H, W) uint8 -> the painted copy."""
    out = np.array(mask, np.uint8, copy=True)
    for b in range(out.shape[0]):
        polys = [(int(poly_label[q]), [tuple(int(x) for x in v) for v in verts[poly_ptr[q]:poly_ptr[q + 1]]])
                 for q in range(int(image_ptr[b]), int(image_ptr[b + 1]))]
        out[b] = apply(out[b], polys, covered)
    return out
