"""Intelligent scissors in plain NumPy with a heapq Dijkstra, written from the contract of ggc_trace_paths in include/ggc.h
(section H4): the box-sum guide, the gradient and the flatness, the windows, the distance to b inside a window and the
walk with its tie rule.  Integers only; this is what the device is compared against, never the other way round."""
from __future__ import annotations

import heapq

import numpy as np

AXIAL, DIAG = 80, 113
UNREACHED = 1 << 30
# N, NE, E, SE, S, SW, W, NW: the order in which the walk looks for its successor
DIRECTIONS = [(-1, 0, AXIAL), (-1, 1, DIAG), (0, 1, AXIAL), (1, 1, DIAG), (1, 0, AXIAL), (1, -1, DIAG), (0, -1, AXIAL),
              (-1, -1, DIAG)]


def guide(bgr: np.ndarray) -> np.ndarray:
    """(H,W,3) uint8 -> (H,W,3) int64: 3x3 box sum with replicated border."""
    p = np.pad(np.asarray(bgr, np.int64), ((1, 1), (1, 1), (0, 0)), mode="edge")
    h, w = bgr.shape[:2]
    return sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))


def gradient(bgr: np.ndarray) -> np.ndarray:
    """(H,W) int64: G, central differences of the box sums with the coordinates clamped into the image."""
    s = guide(bgr)
    h, w = bgr.shape[:2]
    yp, ym = np.minimum(np.arange(h) + 1, h - 1), np.maximum(np.arange(h) - 1, 0)
    xp, xm = np.minimum(np.arange(w) + 1, w - 1), np.maximum(np.arange(w) - 1, 0)
    return (np.abs(s[:, xp] - s[:, xm]) + np.abs(s[yp] - s[ym])).sum(axis=2)


def flatness(bgr: np.ndarray, edge_cap: int) -> np.ndarray:
    """(H,W) int64 in 0..255: 0 on a strong edge, 255 on flat ground."""
    cap = int(edge_cap)
    return ((cap - np.minimum(gradient(bgr), cap)) * 255) // cap


def window(a, b, margin: int, h: int, w: int):
    """(y0, x0, height, width) of segment a -> b."""
    y0, x0 = max(min(a[0], b[0]) - margin, 0), max(min(a[1], b[1]) - margin, 0)
    y1, x1 = min(max(a[0], b[0]) + margin, h - 1), min(max(a[1], b[1]) + margin, w - 1)
    return y0, x0, y1 - y0 + 1, x1 - x0 + 1


def segments(anchors, closed: bool):
    """The (a, b) pairs of a path."""
    pts = [(int(r), int(c)) for r, c in anchors]
    n = len(pts)
    assert n >= (3 if closed else 2)
    return [(pts[i], pts[(i + 1) % n]) for i in range(n if closed else n - 1)]


def distance(flat: np.ndarray, a, b, margin: int, smooth: int):
    """D over the window of segment a -> b: (window, (wh, ww) int32 D), D(p) = cost of the cheapest path inside the window
    from p to b."""
    h, w = flat.shape
    win = window(a, b, margin, h, w)
    y0, x0, wh, ww = win
    f = flat[y0:y0 + wh, x0:x0 + ww].tolist()
    dist = [[UNREACHED] * ww for _ in range(wh)]
    by, bx = b[0] - y0, b[1] - x0
    dist[by][bx] = 0
    heap = [(0, by, bx)]
    while heap:
        d, y, x = heapq.heappop(heap)
        if d != dist[y][x]:
            continue
        base = int(smooth) + f[y][x]
        for dy, dx, length in DIRECTIONS:
            yy, xx = y + dy, x + dx
            if 0 <= yy < wh and 0 <= xx < ww:
                nd = d + length * (base + f[yy][xx])
                if nd < dist[yy][xx]:
                    dist[yy][xx] = nd
                    heapq.heappush(heap, (nd, yy, xx))
    return win, np.asarray(dist, np.int32)


def walk(flat: np.ndarray, win, dist: np.ndarray, a, b, smooth: int):
    """The pixels from a inclusive to b exclusive, image coordinates."""
    y0, x0, wh, ww = win
    y, x = a[0] - y0, a[1] - x0
    by, bx = b[0] - y0, b[1] - x0
    out = []
    while (y, x) != (by, bx):
        out.append((y + y0, x + x0))
        for dy, dx, length in DIRECTIONS:
            yy, xx = y + dy, x + dx
            if 0 <= yy < wh and 0 <= xx < ww and \
                    int(dist[yy, xx]) + length * (int(smooth) + int(flat[y + y0, x + x0]) + int(flat[yy + y0, xx + x0])) == int(dist[y, x]):
                y, x = yy, xx
                break
        else:
            raise AssertionError("the walk found no successor")
    return out


def trace_path(bgr: np.ndarray, anchors, closed: bool, margin: int, edge_cap: int, smooth: int, flat=None, planes=None):
    """The vertices of one path, (n,2) int32.  planes, a list, receives each segment's D, flattened."""
    flat = flatness(bgr, edge_cap) if flat is None else flat
    pts = []
    for a, b in segments(anchors, closed):
        win, dist = distance(flat, a, b, margin, smooth)
        if planes is not None:
            planes.append(dist.ravel())
        pts += walk(flat, win, dist, a, b, smooth)
    if not closed:
        pts.append((int(anchors[-1][0]), int(anchors[-1][1])))
    return np.asarray(pts, np.int32).reshape(-1, 2)


def trace_batch(images, paths_per_image, margin: int, edge_cap: int, smooth: int, planes=None):
    """images: sequence of (H,W,3) uint8; paths_per_image: per image None or a list of (anchors, closed).
    -> (verts (V,2) int32, vert_ptr (Q+1,) int32) in ggc_trace_paths' packing."""
    verts, ptr = [], [0]
    for img, paths in zip(images, paths_per_image):
        if not paths:
            continue
        flat = flatness(img, edge_cap)
        for anchors, closed in paths:
            v = trace_path(img, anchors, closed, margin, edge_cap, smooth, flat, planes)
            verts.append(v)
            ptr.append(ptr[-1] + len(v))
    v = np.concatenate(verts) if verts else np.zeros((0, 2), np.int32)
    return v.astype(np.int32).reshape(-1, 2), np.asarray(ptr, np.int32)


# ---------------------------------------------------------------- the quality study (ISSUE / DESIGN §5.24)

def boundary_anchors(gt: np.ndarray, n: int):
    """The study's anchors on the ground truth's outline: -> (boundary (H,W) bool, [(row, col)] * n).  The largest
    8-connected component with its holes filled; boundary = component minus its 3x3 erosion; anchor k sits at angle
    -pi + 2 pi (k + 1/2) / n about the centre of mass: of the boundary pixels within 0.1 rad of it (the nearest in angle if
    there is none) the one farthest from the centre."""
    from scipy import ndimage
    lab, k = ndimage.label(gt > 0, structure=np.ones((3, 3)))
    sizes = ndimage.sum(gt > 0, lab, range(1, k + 1))
    comp = ndimage.binary_fill_holes(lab == 1 + int(np.argmax(sizes)))
    boundary = comp & ~ndimage.binary_erosion(comp, structure=np.ones((3, 3)))
    cy, cx = ndimage.center_of_mass(comp)
    ys, xs = np.nonzero(boundary)
    ang = np.arctan2(ys - cy, xs - cx)
    rad = np.hypot(ys - cy, xs - cx)
    anchors = []
    for i in range(n):
        t = -np.pi + 2 * np.pi * (i + 0.5) / n
        diff = np.abs((ang - t + np.pi) % (2 * np.pi) - np.pi)
        near = np.nonzero(diff <= 0.1)[0]
        j = near[np.argmax(rad[near])] if len(near) else int(np.argmin(diff))
        anchors.append((int(ys[j]), int(xs[j])))
    return boundary, anchors


def chord_pixels(anchors):
    """The closed polygon's chords sampled at every pixel step (rounded), as the study's baseline."""
    out = []
    n = len(anchors)
    for i in range(n):
        (r0, c0), (r1, c1) = anchors[i], anchors[(i + 1) % n]
        steps = max(abs(r1 - r0), abs(c1 - c0), 1)
        for s in range(steps):
            out.append((int(round(r0 + (r1 - r0) * s / steps)), int(round(c0 + (c1 - c0) * s / steps))))
    return np.asarray(out, np.int32).reshape(-1, 2)


def distance_to_boundary(boundary: np.ndarray, pixels: np.ndarray) -> np.ndarray:
    """Euclidean distance of each pixel to the nearest boundary pixel."""
    from scipy import ndimage
    edt = ndimage.distance_transform_edt(~boundary)
    return edt[pixels[:, 0], pixels[:, 1]]


def study_rows(scenes=range(30000, 30008), counts=(4, 6, 8), margin=16, edge_cap=2048, smooth=16, h=120, w=160):
    """-> [(n, traced mean, chords mean, traced worst, chords worst)], the means averaged over the scenes."""
    from gcn_grabcut.synthetic import synthetic_image
    rows = []
    data = [synthetic_image(h, w, s, return_mask=True) for s in scenes]
    for n in counts:
        tm, cm, tw, cw = [], [], [], []
        for img, gt in data:
            boundary, anchors = boundary_anchors(gt, n)
            dt = distance_to_boundary(boundary, trace_path(img, anchors, True, margin, edge_cap, smooth))
            dc = distance_to_boundary(boundary, chord_pixels(anchors))
            tm.append(dt.mean()); cm.append(dc.mean()); tw.append(dt.max()); cw.append(dc.max())
        rows.append((n, float(np.mean(tm)), float(np.mean(cm)), float(np.max(tw)), float(np.max(cw))))
    return rows
