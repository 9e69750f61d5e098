"""The magic wand of include/ggc.h H5 in Python integers and numpy: the reference the device is held to.

The component of a seed is found by a plain queue flood fill from the seed's pixel; deliberately not a union-find."""
from collections import deque

import numpy as np

GGC_BGD, GGC_FGD = 0, 1


def ref_sums(img, r, c, n):
    """The three reference sums of the seed at (r, c): the n x n bytes around it, the border replicated."""
    h, w = img.shape[:2]
    half = n // 2
    out = [0, 0, 0]
    for dy in range(-half, half + 1):
        y = min(max(r + dy, 0), h - 1)
        for dx in range(-half, half + 1):
            x = min(max(c + dx, 0), w - 1)
            for ch in range(3):
                out[ch] += int(img[y, x, ch])
    return out


def match_one(px, ref, tolerance, n):
    """match(p, s) for one pixel's three bytes."""
    return all(abs(n * n * int(px[ch]) - ref[ch]) <= n * n * tolerance for ch in range(3))


def match_plane(img, ref, tolerance, n):
    """(H, W) bool: match(p, s) for every pixel."""
    d = np.abs(n * n * img.astype(np.int64) - np.asarray(ref, np.int64)[None, None, :])
    return (d <= n * n * tolerance).all(axis=2)


def flood(on, r, c, connectivity):
    """The 4- or 8-connected component of (r, c) within the bool plane `on`, by a queue; empty when (r, c) is off."""
    h, w = on.shape
    sel = np.zeros((h, w), bool)
    if not on[r, c]:
        return sel
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if connectivity == 8:
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    sel[r, c] = True
    queue = deque([(r, c)])
    while queue:
        y, x = queue.popleft()
        for dy, dx in steps:
            yy, xx = y + dy, x + dx
            if 0 <= yy < h and 0 <= xx < w and on[yy, xx] and not sel[yy, xx]:
                sel[yy, xx] = True
                queue.append((yy, xx))
    return sel


def selection(img, r, c, tolerance, connectivity, sample):
    """Sel(s) of the seed at (r, c) of one (H, W, 3) uint8 image, as a bool plane; the seed must be inside."""
    on = match_plane(img, ref_sums(img, r, c, sample), tolerance, sample)
    return on if connectivity == 0 else flood(on, r, c, connectivity)


def wand_image(img, seeds, tolerance, connectivity, sample, mask=None):
    """One image: seeds = rows (row, col, label) in seed order -> (mask or None, select, counts).  A pixel is decided by
    the last seed whose selection holds it; a seed outside the image is ignored."""
    h, w = img.shape[:2]
    decided = np.zeros((h, w), np.uint8)           # 0 none, 1 background, 2 foreground
    for r, c, label in seeds:
        r, c = int(r), int(c)
        if not (0 <= r < h and 0 <= c < w):
            continue
        decided[selection(img, r, c, tolerance, connectivity, sample)] = 2 if label != 0 else 1
    select = np.where(decided == 2, 255, 0).astype(np.uint8)
    counts = np.array([(decided == 2).sum(), (decided == 1).sum()], np.int32)
    out = None
    if mask is not None:
        out = np.array(mask, np.uint8, copy=True)
        out[decided == 2] = GGC_FGD
        out[decided == 1] = GGC_BGD
    return out, select, counts


def wand_batch(imgs, seeds, seed_ptr, tolerance, connectivity, sample, mask=None):
    """A batch: imgs (B, H, W, 3), seeds (K, 3), seed_ptr (B + 1,) -> (mask (B, H, W) or None, select (B, H, W),
    counts (B, 2))."""
    outs = [wand_image(imgs[b], np.asarray(seeds).reshape(-1, 3)[int(seed_ptr[b]):int(seed_ptr[b + 1])], tolerance,
                       connectivity, sample, None if mask is None else mask[b]) for b in range(len(imgs))]
    return (None if mask is None else np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]),
            np.stack([o[2] for o in outs]))
