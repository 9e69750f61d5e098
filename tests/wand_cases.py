"""Byte images for the magic-wand tests: two or three grey levels in patterns whose components are known to be awkward
for a run-based union-find (diagonals, combs, a spiral, a ring), with a noisy variant of each, and seeded random images
quantised to a few levels per channel."""
import numpy as np

LEVELS = np.array([[30, 60, 90], [200, 180, 160], [110, 120, 130]], np.uint8)     # BGR of level 0, 1, 2
NOISE = 3                                                                          # the noisy variant adds 0..NOISE per byte


def to_image(plane, noisy=False, seed=0):
    """(H, W) plane of levels 0..2 -> (H, W, 3) uint8; noisy: plus 0..NOISE per byte, so a tolerance of NOISE still
    separates the levels (they are at least 60 apart) while no two pixels of a level need be equal."""
    img = LEVELS[np.asarray(plane, np.int64)]
    if noisy:
        img = img + np.random.default_rng(seed).integers(0, NOISE + 1, img.shape).astype(np.uint8)
    return np.ascontiguousarray(img, np.uint8)


def diagonal(h, w, down=True):
    """A line one pixel wide from a top corner: 8-connected, not 4-connected."""
    p = np.zeros((h, w), np.uint8)
    for y in range(h):
        x = y if down else w - 1 - y
        if 0 <= x < w:
            p[y, x] = 1
    return p


def staircase(h, w, down=True):
    """Steps two pixels wide: 4-connected."""
    p = diagonal(h, w, down)
    for y in range(h):
        x = y + 1 if down else w - 2 - y
        if 0 <= x < w:
            p[y, x] = 1
    return p


def comb(h, w):
    p = np.zeros((h, w), np.uint8)
    p[0, :] = 1
    p[:, ::2] = 1
    return p


def spiral(n):
    """One pixel wide, from the top-left corner inwards: one long component, and its complement another."""
    g = np.zeros((n, n), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    g[0, 0] = 1
    turns = 0
    while turns < 2:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if 0 <= ny < n and 0 <= nx < n and not g[ny, nx] and not (0 <= ay < n and 0 <= ax < n and g[ay, ax]):
            y, x = ny, nx
            g[y, x] = 1
            turns = 0
        else:
            dy, dx = dx, -dy
            turns += 1
    return g


def ring(h, w):
    """Level 0 outside and inside a closed ring of level 1: the inside matches an outside seed but is not connected."""
    p = np.zeros((h, w), np.uint8)
    p[1:h - 1, 1:w - 1] = 1
    p[2:h - 2, 2:w - 2] = 0
    return p


def blocky(rng, h, w, levels=3, block=4):
    """Random levels in blocks: components of every shape."""
    small = rng.integers(0, levels, (-(-h // block), -(-w // block)))
    return np.kron(small, np.ones((block, block), np.int64))[:h, :w].astype(np.uint8)


def quantised(rng, h, w, levels):
    """A random image with `levels` values per channel, each channel drawn on its own in blocks of 1..3 pixels."""
    step = 255 // max(levels - 1, 1)
    block = int(rng.integers(1, 4))
    chans = [blocky(rng, h, w, levels, block).astype(np.int64) * step for _ in range(3)]
    return np.ascontiguousarray(np.stack(chans, axis=2).astype(np.uint8))


def pack(per_image):
    """per_image: for every image a list of (row, col, label) in seed order -> (seeds (K, 3) int32, seed_ptr (B + 1,))."""
    rows = [s for seeds in per_image for s in seeds]
    ptr = np.concatenate([[0], np.cumsum([len(seeds) for seeds in per_image])]).astype(np.int32)
    return np.asarray(rows, np.int32).reshape(-1, 3), ptr
