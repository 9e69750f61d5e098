"""The masks the distance-transform tests share (tests/test_distance_gpu.py, test_modify_mask_gpu.py,
test_distance_fuzz_gpu.py), and their references from tests/distance_ref.py, computed once per (shape, mask, border flag)."""
import functools

import numpy as np

import distance_ref as ref

THIN = (1, 63, 64, 65, 257)
SHAPES = [(1, 1)] + [(1, w) for w in THIN[1:]] + [(h, 1) for h in THIN[1:]] + [(7, 5), (64, 64), (65, 129), (33, 300)]
KINDS = ("full", "empty", "hole_in_corner", "dot_in_corner", "checkerboard", "frame", "two_disks", "ring25",
         "noise_0.01", "noise_0.5", "noise_0.99")
CAPS = (0, 1, 2, 25, 26)
RING25 = [(dy, dx) for dy in range(-5, 6) for dx in range(-5, 6) if dy * dy + dx * dx == 25]      # (3, 4), (5, 0) and their images


def disk(shape, cy, cx, r2):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    return (y - cy) ** 2 + (x - cx) ** 2 <= r2


@functools.lru_cache(maxsize=None)
def mask(shape, kind):
    """One (H, W) uint8 mask; set pixels are 1.  hole_in_corner and dot_in_corner are the unbounded walk's worst case; ring25
    is background whose centre pixel has its nearest foreground at exactly d2 = 25."""
    h, w = shape
    m = np.zeros(shape, np.uint8)
    if kind == "full":
        m[:] = 1
    elif kind == "hole_in_corner":
        m[:] = 1
        m[0, 0] = 0
    elif kind == "dot_in_corner":
        m[h - 1, w - 1] = 1
    elif kind == "checkerboard":
        m[:] = np.add.outer(np.arange(h), np.arange(w)) % 2 == 0
    elif kind == "frame":
        m[0, :] = m[-1, :] = 1
        m[:, 0] = m[:, -1] = 1
    elif kind == "two_disks":
        m[:] = disk(shape, h // 3, w // 4, (min(h, w) // 3) ** 2) | disk(shape, (2 * h) // 3, (3 * w) // 4, max(h, w) // 5)
    elif kind == "ring25":
        for dy, dx in RING25:
            y, x = h // 2 + dy, w // 2 + dx
            if 0 <= y < h and 0 <= x < w:
                m[y, x] = 1
    elif kind.startswith("noise_"):
        rng = np.random.default_rng(h * 1000 + w)
        m[:] = rng.random(shape) < float(kind[6:])
    elif kind != "empty":
        raise ValueError(kind)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def unbounded(shape, kind, border):
    """The reference's unbounded signed d2 of mask(shape, kind); a capped one is ref.apply_cap of it."""
    d = ref.signed_d2(mask(shape, kind), border, 0)
    d.setflags(write=False)
    return d


def fuzz_mask(rng, h, w):
    """One mask of a random kind: those above, random rectangles, blobs (a thresholded smooth field)."""
    kind = int(rng.integers(0, 8))
    m = np.zeros((h, w), np.uint8)
    if kind == 0:
        m[:] = rng.integers(0, 2)
    elif kind == 1:
        m[:] = rng.random((h, w)) < rng.choice([0.01, 0.5, 0.99])
    elif kind == 2:
        m[:] = np.add.outer(np.arange(h), np.arange(w)) % 2 == rng.integers(0, 2)
    elif kind == 3:
        m[:] = 1 - rng.integers(0, 2)
        m[rng.integers(0, h), rng.integers(0, w)] ^= 1                  # one pixel of the other class
    elif kind in (4, 5):
        for _ in range(int(rng.integers(1, 5))):
            y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            m[y0:y0 + int(rng.integers(1, h + 1)), x0:x0 + int(rng.integers(1, w + 1))] ^= 1
    else:
        f = rng.random((h + 8, w + 8))
        f = sum(np.roll(np.roll(f, dy, 0), dx, 1) for dy in range(-3, 4) for dx in range(-3, 4))[4:4 + h, 4:4 + w]
        m[:] = f > np.quantile(f, rng.choice([0.3, 0.6, 0.9]))
    return m * rng.choice(np.array([1, 7, 255], np.uint8))
