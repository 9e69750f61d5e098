"""Geodesic click hints in plain NumPy with a heapq Dijkstra, written from the contract of ggc_geodesic_hints in
include/ggc.h (section H1): the box-sum guide, the sources with last-click-wins, the capped distances, the label rule and
the per-superpixel minima.  Integers only; this is what the device is compared against, never the other way round."""
from __future__ import annotations

import heapq

import numpy as np

AXIAL, DIAG = 80, 113
FGD, BGD = 1, 0
_NEIGHBOURS = [(-1, 0, AXIAL), (1, 0, AXIAL), (0, -1, AXIAL), (0, 1, AXIAL),
               (-1, -1, DIAG), (-1, 1, DIAG), (1, -1, DIAG), (1, 1, DIAG)]


def guide(bgr: np.ndarray) -> np.ndarray:
    """(H,W,3) uint8 -> (H,W,3) int64: 3x3 box sum with replicated border."""
    p = np.pad(np.asarray(bgr, np.int64), ((1, 1), (1, 1), (0, 0)), mode="edge")
    h, w = bgr.shape[:2]
    return sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))


def sources(h: int, w: int, fg_points, bg_points):
    """pack_hints' click order (foreground clicks, then background clicks); out-of-frame clicks are dropped and the last
    click on a pixel decides its label.  Returns (foreground pixels, background pixels), disjoint."""
    clicks = [(int(r), int(c), 1) for r, c in (fg_points or [])] + [(int(r), int(c), 0) for r, c in (bg_points or [])]
    return sources_from_rows(h, w, clicks)


def sources_from_rows(h: int, w: int, rows):
    """rows of (row, col, label) in click order, label != 0 = foreground."""
    last = {}
    for r, c, l in rows:
        r, c = int(r), int(c)
        if 0 <= r < h and 0 <= c < w:
            last[(r, c)] = 1 if int(l) != 0 else 0
    return [p for p, l in last.items() if l == 1], [p for p, l in last.items() if l == 0]


def distances(bgr: np.ndarray, srcs, radius: int, gamma: int) -> np.ndarray:
    """(H,W) int32: min(D, limit + 1), D the cheapest path cost to the nearest pixel of srcs."""
    h, w = bgr.shape[:2]
    limit = AXIAL * int(radius)
    s = guide(bgr)
    dist = np.full((h, w), limit + 1, np.int64)
    heap = []
    for r, c in srcs:
        dist[r, c] = 0
        heap.append((0, r, c))
    heapq.heapify(heap)
    while heap:
        d, y, x = heapq.heappop(heap)
        if d != dist[y, x]:
            continue
        for dy, dx, length in _NEIGHBOURS:
            yy, xx = y + dy, x + dx
            if 0 <= yy < h and 0 <= xx < w:
                nd = d + length + int(gamma) * int(np.abs(s[y, x] - s[yy, xx]).sum())
                if nd <= limit and nd < dist[yy, xx]:
                    dist[yy, xx] = nd
                    heapq.heappush(heap, (nd, yy, xx))
    return dist.astype(np.int32)


def geodesic_ref(bgr, fg_points, bg_points, radius, gamma, mask=None, segments=None, rows=None):
    """One image.  Returns a dict: dist_fg, dist_bg (H,W) int32; mask (the painted copy, when one is given); node_dist
    (n,2) int32 with n = segments.max() + 1 (when segments is given).  rows, if given, replaces the two point lists by
    (row, col, label) rows in click order."""
    h, w = bgr.shape[:2]
    fg, bg = sources_from_rows(h, w, rows) if rows is not None else sources(h, w, fg_points, bg_points)
    limit = AXIAL * int(radius)
    df, db = distances(bgr, fg, radius, gamma), distances(bgr, bg, radius, gamma)
    out = {"dist_fg": df, "dist_bg": db}
    if mask is not None:
        m = np.array(mask, np.uint8, copy=True)
        m[(df <= limit) & (df < db)] = FGD
        m[(db <= limit) & (db < df)] = BGD
        out["mask"] = m
    if segments is not None:
        n = int(segments.max()) + 1
        nd = np.full((n, 2), limit + 1, np.int32)
        np.minimum.at(nd[:, 0], segments.ravel(), df.ravel())
        np.minimum.at(nd[:, 1], segments.ravel(), db.ravel())
        out["node_dist"] = nd
    return out


def definite_labels(bgr, fg_points, bg_points, radius, gamma, rows=None) -> np.ndarray:
    """(H,W) int: 1 / 0 where the rule paints foreground / background, -1 where it paints nothing."""
    m = geodesic_ref(bgr, fg_points, bg_points, radius, gamma, mask=np.full(bgr.shape[:2], 255, np.uint8), rows=rows)["mask"]
    lab = m.astype(np.int32)
    lab[lab == 255] = -1
    return lab


def serpentine(h: int = 70, w: int = 70) -> np.ndarray:
    """Value 200 with horizontal walls of colour (20,30,40), 3 rows thick, every 6 rows from row 3, each open for 4 columns
    alternately at the right and the left end."""
    img = np.full((h, w, 3), 200, np.uint8)
    for i, y in enumerate(range(3, h - 2, 6)):
        img[y:y + 3] = (20, 30, 40)
        if i % 2 == 0:
            img[y:y + 3, w - 4:] = 200
        else:
            img[y:y + 3, :4] = 200
    return img
