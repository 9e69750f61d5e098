"""Raw label maps for the tile-local path of ggc_slic_enforce_connectivity, shared by the CPU test that pins
which path each map must take and the GPU tests that run them.  No device code is used here: expected_path counts the
4-connected components of each raw label with scipy.ndimage.label.

Paths, as the profiler scopes of the library name them:
    "tiles"   slic_cn_tiles (and slic_cn_replay if there is a small component), nothing else
    "spill"   the same and slic_cn_spill: a component below min_size has more pixels than the on-chip queue holds
    "rounds"  slic_cn_tiles, then slic_cn_rounds from the start: a component has max_size pixels or more
"""
import hashlib

import numpy as np

TW, TH = 64, 16          # CN_TW, CN_TH of csrc/ggc_slic.hip
QCAP = 256               # CN_QCAP
BIG = 10 ** 6
SCOPES = ("slic_cn_tiles", "slic_cn_replay", "slic_cn_spill", "slic_cn_rounds")


def component_sizes(raw):
    """Sizes of the 4-connected components of equal raw label of one image."""
    from scipy import ndimage
    sizes = []
    for v in np.unique(raw):
        lab, n = ndimage.label(raw == v)
        sizes.extend(np.bincount(lab.ravel())[1:].tolist())
    return sizes


def expected_path(raw, mn, mx):
    sizes = [s for img in raw for s in component_sizes(img)]
    if any(s >= max(mx, 1) for s in sizes):
        return "rounds"
    if any(QCAP < s < mn for s in sizes):
        return "spill"
    return "tiles"


def scopes_of(path, knob_on=True):
    """scope -> whether it must have been recorded (None: either)."""
    if not knob_on:
        return {"slic_cn_tiles": False, "slic_cn_replay": False, "slic_cn_spill": False, "slic_cn_rounds": True}
    return {"slic_cn_tiles": True, "slic_cn_replay": False if path == "rounds" else None,
            "slic_cn_spill": path == "spill", "slic_cn_rounds": path == "rounds"}


# ------------------------------------------------------------------ generators

def noise(b, h, w, seed, labels=3):
    return np.random.default_rng(seed).integers(0, labels, (b, h, w)).astype(np.int32)


def speckled_blocks(b, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = ((yy // 9) * 2 + (xx // 11) * 3) % 5
    raw = np.repeat(base[None], b, axis=0).astype(np.int32)
    speck = rng.random((b, h, w)) < 0.08
    raw[speck] = 5 + rng.integers(0, 3, int(speck.sum()))
    return raw


def cut_stripes(b, h, w, seed):
    """Vertical stripes one to three pixels wide, cut across at random rows."""
    rng = np.random.default_rng(seed)
    raw = np.zeros((b, h, w), np.int32)
    for i in range(b):
        x, lab = 0, 0
        while x < w:
            wd = int(rng.integers(1, 4))
            raw[i, :, x:x + wd] = lab % 3
            for y in np.flatnonzero(rng.random(h) < 0.07):
                raw[i, y, x:x + wd] = 3 + lab % 2
            x += wd
            lab += 1
    return raw


def walk_blobs(b, h, w, seed):
    """Random-walk blobs of their own labels on a sea of label 0."""
    rng = np.random.default_rng(seed)
    raw = np.zeros((b, h, w), np.int32)
    for i in range(b):
        for k in range(int(rng.integers(3, 12))):
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            for _ in range(int(rng.integers(1, 400))):
                raw[i, y, x] = 1 + k % 4
                dy, dx = ((0, 1), (0, -1), (1, 0), (-1, 0))[int(rng.integers(0, 4))]
                y, x = min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)
    return raw


def serpentine(h, w, length):
    """A one-pixel-wide path of `length` pixels of label 1 that snakes through a sea of label 0."""
    raw = np.zeros((h, w), np.int32)
    y, x, step, left = 1, 1, 1, length
    while left:
        assert y < h - 1, "map too small for the path"
        raw[y, x] = 1
        left -= 1
        if 1 <= x + step <= w - 2:
            x += step
        else:
            if left:
                raw[y + 1, x] = 1
                left -= 1
            y += 2
            step = -step
    return raw


def spiral(h, w):
    """A one-pixel-wide spiral of label 1 from the top left corner inwards, one pixel of sea between its turns."""
    raw = np.zeros((h, w), np.int32)
    y, x, dy, dx = 1, 1, 0, 1
    raw[y, x] = 1

    def free(yy, xx):
        return 1 <= yy <= h - 2 and 1 <= xx <= w - 2 and raw[yy, xx] == 0

    def ahead_clear(yy, xx):
        return not (0 <= yy < h and 0 <= xx < w) or raw[yy, xx] == 0

    while True:
        for _ in range(2):
            if free(y + dy, x + dx) and ahead_clear(y + 2 * dy, x + 2 * dx):
                break
            dy, dx = dx, -dy                                        # clockwise: right, down, left, up
        else:
            return raw
        y, x = y + dy, x + dx
        raw[y, x] = 1


def u_shape():
    """Arms in the first tile row, the bend in the second: the arms are one component only through the tile below."""
    raw = np.zeros((2 * TH + 3, TW + 9), np.int32)
    raw[3:TH + 2, 5] = 1
    raw[3:TH + 2, 11] = 1
    raw[TH + 1, 5:12] = 1
    return raw


def last_column_root():
    """A component whose smallest raster index lies in the last tile column and whose bulk lies in the first."""
    h, w = 2 * TH + 5, 2 * TW + 12
    raw = np.zeros((h, w), np.int32)
    raw[0:TH + 5, 2 * TW + 2] = 1
    raw[TH + 4, 3:2 * TW + 3] = 1
    raw[2:TH + 5, 3] = 1
    raw[2, 3:40] = 1
    return raw


def checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy + xx) % 2).astype(np.int32)


def blobs_on_stripes(vertical):
    """Stripes three pixels wide, each a kept component, with small components of other labels laid over several of them:
    which stripe a small component is absorbed into is decided by the order of its breadth-first replay.  One blob lies on
    the corner where four tiles meet, two have min_size - 1 = 39 and min_size = 40 pixels, and a row of touching 3 x 3
    squares of different labels makes a chain in which each is absorbed into the one before it."""
    h, w = 3 * TH + 4, 2 * TW + 20
    yy, xx = np.mgrid[0:h, 0:w]
    raw = (((xx if vertical else yy) // 3) % 3).astype(np.int32)
    raw[TH - 2:TH + 3, TW - 3:TW + 4] = 9                           # 5 x 7 across the tile corner (TH, TW)
    raw[3:8, 10:18] = 10                                            # 40 pixels: kept
    stripe = raw[3, 30]
    raw[3:8, 30:38] = 11
    raw[3, 30] = stripe                                             # 39 pixels: absorbed
    for k in range(5):                                              # the chain
        raw[2 * TH + 2:2 * TH + 5, 20 + 3 * k:23 + 3 * k] = 12 + k
    for k in range(4):                                              # a diagonal chain, roots on different rows
        raw[22 + 2 * k:24 + 2 * k, 90 + 2 * k:93 + 2 * k] = 20 + k
    raw[10:13, TW + 30:TW + 41] = 30                                # an L and a plus: fronts that turn
    raw[10:20, TW + 30] = 30
    raw[36, TW + 40:TW + 47] = 31
    raw[33:40, TW + 43] = 31
    return raw


def hand_cases():
    """name -> (raw [B,H,W], min_size, max_size, path)"""
    cases = {
        "u_shape": (u_shape()[None], 4, BIG, "tiles"),
        "spiral": (spiral(3 * TH + 3, 3 * TW + 5)[None], 30, BIG, "tiles"),
        "spiral_absorbed": (spiral(2 * TH + 3, 2 * TW + 5)[None], 3000, BIG, "spill"),
        "serpentine_across_tiles": (serpentine(40, 150, 1500)[None], 30, BIG, "tiles"),
        "last_column_root": (last_column_root()[None], 4, BIG, "tiles"),
        "checkerboard_absorbed": (checkerboard(40, 130)[None], 3, BIG, "tiles"),
        "checkerboard_kept": (checkerboard(40, 130)[None], 1, BIG, "tiles"),
        "blobs_on_vertical_stripes": (blobs_on_stripes(True)[None], 40, BIG, "tiles"),
        "blobs_on_horizontal_stripes": (blobs_on_stripes(False)[None], 40, BIG, "tiles"),
        "batch_of_five": (np.stack([noise(1, 40, 150, 1)[0], serpentine(40, 150, 90), speckled_blocks(1, 40, 150, 2)[0],
                                    cut_stripes(1, 40, 150, 3)[0], walk_blobs(1, 40, 150, 4)[0]]), 20, BIG, "tiles"),
        "batch_of_one": (walk_blobs(1, 40, 150, 5), 20, BIG, "tiles"),
        "carved_blocks": (speckled_blocks(2, 40, 150, 6), 20, 60, "rounds"),
    }
    return cases


FUZZ_KINDS = (lambda b, h, w, s: noise(b, h, w, s, 2 + s % 3), speckled_blocks, cut_stripes, walk_blobs)
FUZZ_SEED0 = 1000


def fuzz_case(k):
    """Case k of 40: batch 2-4, height 1-80, width 1-150, the four kinds in turn."""
    rng = np.random.default_rng(FUZZ_SEED0 + k)
    b, h, w = int(rng.integers(2, 5)), int(rng.integers(1, 81)), int(rng.integers(1, 151))
    mn = int(rng.choice([4, 20, 100, 300]))
    mx = int(rng.choice([3 * mn, BIG]))
    return FUZZ_KINDS[k % 4](b, h, w, FUZZ_SEED0 + k), mn, mx


# which path each fuzz case takes, counted by test_connectivity_cases_cpu.py with scipy and asserted on the device
FUZZ_PATHS = tuple({"t": "tiles", "r": "rounds", "s": "spill"}[c] for c in "tttrtttttttttttrtttrrttttttttttrrttrttrt")


def digest(out, n):
    return hashlib.sha1(np.ascontiguousarray(out, np.int32).tobytes() + np.ascontiguousarray(n, np.int32).tobytes()).hexdigest()
