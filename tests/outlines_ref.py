"""Mask outlines (include/ggc.h K1) restated in plain Python integers, from the header's text and not from the kernels.

Corners (r, c), 0 <= r <= H, 0 <= c <= W; pixel (y, x) is the unit square between corners (y, x) and (y+1, x+1); anything
outside the image is background.  A crack is a directed unit step with a foreground pixel on its right and a background
pixel on its left; directions 0 = E, 1 = S, 2 = W, 3 = N; key = ((r (W+1) + c) 4 + d) of its tail.  The successor of a
crack arriving at a corner in direction d is the first existing crack leaving it among left, straight, right (connectivity
8) or right, straight, left (4).  The cycles of the successor are the loops; a loop starts at its smallest key; its
vertices are the tails of the cracks whose predecessor has another direction."""
import numpy as np

STEP = ((0, 1), (1, 0), (0, -1), (-1, 0))          # E S W N as (dr, dc)


def _fg(mask, y, x):
    h, w = mask.shape
    return 0 <= y < h and 0 <= x < w and mask[y, x] != 0


def leaves(mask, r, c, d):
    """Does a crack leave corner (r, c) in direction d?"""
    if d == 0:
        return _fg(mask, r, c) and not _fg(mask, r - 1, c)
    if d == 1:
        return _fg(mask, r, c - 1) and not _fg(mask, r, c)
    if d == 2:
        return _fg(mask, r - 1, c - 1) and not _fg(mask, r, c - 1)
    return _fg(mask, r - 1, c) and not _fg(mask, r - 1, c - 1)


def successor(mask, r, c, d, connectivity):
    """The crack after (r, c, d): (r', c', d')."""
    hr, hc = r + STEP[d][0], c + STEP[d][1]
    order = ((d + 3) & 3, d, (d + 1) & 3) if connectivity == 8 else ((d + 1) & 3, d, (d + 3) & 3)
    for e in order:
        if leaves(mask, hr, hc, e):
            return hr, hc, e
    raise AssertionError(f"crack {(r, c, d)} has no successor")


def cracks(mask):
    """Every crack as (r, c, d), in key order."""
    h, w = mask.shape
    return [(r, c, d) for r in range(h + 1) for c in range(w + 1) for d in range(4) if leaves(mask, r, c, d)]


def _right_pixel(r, c, d):
    return ((r, c), (r, c - 1), (r - 1, c - 1), (r - 1, c))[d]


def _components(mask, connectivity):
    """label (H, W) int, -1 on background, by flood fill in raster order under `connectivity`."""
    h, w = mask.shape
    lab = -np.ones((h, w), np.int64)
    nb = [(0, 1), (1, 0), (0, -1), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    n = 0
    for y in range(h):
        for x in range(w):
            if mask[y, x] and lab[y, x] < 0:
                lab[y, x] = n
                stack = [(y, x)]
                while stack:
                    a, b = stack.pop()
                    for dy, dx in nb:
                        p, q = a + dy, b + dx
                        if 0 <= p < h and 0 <= q < w and mask[p, q] and lab[p, q] < 0:
                            lab[p, q] = n
                            stack.append((p, q))
                n += 1
    return lab, n


def trace(mask, connectivity=8):
    """One image -> its loops in start-key order, each a dict: vertices [(r, c), ...], area, outer, perimeter, start (r, c, d)."""
    mask = np.asarray(mask)
    assert mask.ndim == 2 and connectivity in (4, 8)
    w = mask.shape[1]
    seen = set()
    loops = []
    for start in cracks(mask):                     # key order: the first unseen crack of a loop is its smallest key
        if start in seen:
            continue
        chain = []
        cur = start
        while cur not in seen:
            seen.add(cur)
            chain.append(cur)
            cur = successor(mask, *cur, connectivity)
        assert cur == start, "successor is not a permutation"
        n = len(chain)
        verts = [(r, c) for i, (r, c, d) in enumerate(chain) if chain[i - 1][2] != d]
        twice = sum(verts[i][1] * verts[(i + 1) % len(verts)][0] - verts[(i + 1) % len(verts)][1] * verts[i][0]
                    for i in range(len(verts)))
        assert twice % 2 == 0
        loops.append({"vertices": verts, "area": twice // 2, "perimeter": n, "start": start, "cracks": chain})
    lab, _ = _components(mask, connectivity)
    comp = [int(lab[_right_pixel(*lp["start"])]) for lp in loops]
    outer_of = {comp[i]: i for i, lp in enumerate(loops) if lp["area"] > 0}
    for i, lp in enumerate(loops):
        lp["outer"] = outer_of[comp[i]]
        lp["key"] = (lp["start"][0] * (w + 1) + lp["start"][1]) * 4 + lp["start"][2]
    return loops


def pack(per_image):
    """Loops per image -> the five arrays of ggc_mask_outlines: verts (V, 2), loop_ptr (Q+1,), loop_info (Q, 3) = area,
    outer, perimeter, image_ptr (B+1,), image_vert_ptr (B+1,), all int32."""
    verts, loop_ptr, info, image_ptr, image_vert_ptr = [], [0], [], [0], [0]
    for loops in per_image:
        for lp in loops:
            verts += lp["vertices"]
            loop_ptr.append(len(verts))
            info.append((lp["area"], lp["outer"], lp["perimeter"]))
        image_ptr.append(len(info))
        image_vert_ptr.append(len(verts))
    return (np.array(verts, np.int32).reshape(-1, 2), np.array(loop_ptr, np.int32), np.array(info, np.int32).reshape(-1, 3),
            np.array(image_ptr, np.int32), np.array(image_vert_ptr, np.int32))


def trace_batch(masks, connectivity=8):
    return pack([trace(m, connectivity) for m in masks])


def fill_back(shape, loops, covered):
    """The XOR of the even-odd fills of the loops, on the doubled grid (2H+1) x (2W+1) by H3's rule (`covered` is
    polygons_ref.covered or covered_np), read at the odd positions: an odd point is never on an edge."""
    h, w = shape
    acc = np.zeros((2 * h + 1, 2 * w + 1), bool)
    for lp in loops:
        verts = lp["vertices"] if isinstance(lp, dict) else lp
        acc ^= covered((2 * h + 1, 2 * w + 1), [(2 * int(r), 2 * int(c)) for r, c in verts])
    return acc[1::2, 1::2]


def check_properties(mask, loops, connectivity, covered=None):
    """Asserts what K1 promises of `loops` = trace(mask, connectivity)."""
    mask = np.asarray(mask) != 0
    h, w = mask.shape
    assert sum(lp["perimeter"] for lp in loops) == len(cracks(mask))
    assert [lp["key"] for lp in loops] == sorted(lp["key"] for lp in loops)
    tails = set()
    for lp in loops:
        r, c, d = lp["start"]
        chain = lp["cracks"]
        corners = [(a, b) for a, b, _ in chain]
        assert (r, c) == min(corners), "the start's tail is the loop's smallest corner"
        assert corners.count((r, c)) == 1, "the loop visits its start corner once"
        assert chain[-1][2] != d, "the loop turns at its start"
        assert (r, c) not in tails, "no other loop starts at the same corner"
        tails.add((r, c))
        assert d == (0 if lp["area"] > 0 else 1), "E for an outer loop, S for a hole"
        assert lp["area"] != 0 and len(lp["vertices"]) >= 4 and len(lp["vertices"]) % 2 == 0
        assert lp["vertices"][0] == (r, c)
    assert sum(lp["area"] for lp in loops) == int(mask.sum())
    _, n_fg = _components(mask, connectivity)
    assert sum(lp["area"] > 0 for lp in loops) == n_fg
    padded = np.ones((h + 2, w + 2), bool)
    padded[1:-1, 1:-1] = ~mask
    lab, n_bg = _components(padded, 4 if connectivity == 8 else 8)
    assert sum(lp["area"] < 0 for lp in loops) == n_bg - 1          # all but the component of the padded border
    for i, lp in enumerate(loops):
        o = loops[lp["outer"]]
        assert o["area"] > 0 and (lp["area"] < 0 or lp["outer"] == i)
    if covered is not None:
        assert np.array_equal(fill_back((h, w), loops, covered), mask)
