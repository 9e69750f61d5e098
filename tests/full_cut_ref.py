"""Numpy restatement of the full-resolution banded cut (test infrastructure): ggc_lift_labels over
upsample_ref.source_coords and closed_form_ref.unknown_band, and cut_mask_full as a chain of the CPU oracle's entries.

    lift    per output pixel (y, x) of (H1, W1): (y0, y1, wy), (x0, x1, wx) = upsample_ref.source_coords (the half-pixel
            formula of ggc_upsample_matte); m = (mask != 0) as float64; v = lerp(lerp(m00, m01, wx), lerp(m10, m11, wx),
            wy), lerp(u, v, t) = u + t (v - u); M1 = (v >= 0.5); U = closed_form_ref.unknown_band(M1, band), the pixels
            within Chebyshev distance band of a pixel whose 3x3 neighbourhood (clipped) holds both values of M1;
            labels = 3 on U and M1, 2 on U off M1, 1 on M1 off U, else 0
    chain   lift -> oracle.convert_color8 (colour spaces other than rgb) -> oracle.grabcut(mode 0, n_iter, seed) from
            the labels -> oracle.clean_mask

scene, working_masks and the baselines below are what tools/full_cut_study.py and the tests run."""
from __future__ import annotations

import math

import numpy as np

from closed_form_ref import unknown_band
from upsample_ref import _coord, _lerp, source_coords, upsample_ref

BAND_MAX = 64


def default_band(shape, full_shape) -> int:
    """min(64, max(1, ceil(1.5 max(H1 / H, W1 / W)))): one and a half working pixels."""
    ratio = max(full_shape[0] / shape[0], full_shape[1] / shape[1])
    return min(BAND_MAX, max(1, math.ceil(1.5 * ratio)))


def lifted_value(mask: np.ndarray, full_shape) -> np.ndarray:
    """(H1, W1) float64: the bilinear interpolation of (mask != 0)."""
    m = (np.asarray(mask) != 0).astype(np.float64)
    h, w = m.shape
    h1, w1 = full_shape
    y0, y1, wy = source_coords(h1, h)
    x0, x1, wx = source_coords(w1, w)
    top = _lerp(m[y0][:, x0], m[y0][:, x1], wx[None, :])
    bot = _lerp(m[y1][:, x0], m[y1][:, x1], wx[None, :])
    return _lerp(top, bot, wy[:, None])


def lift_labels(mask: np.ndarray, full_shape, band: int):
    """-> (labels (H1, W1) uint8 in {0, 1, 2, 3}, mask_full (H1, W1) uint8 in {0, 1})."""
    m1 = lifted_value(mask, full_shape) >= 0.5
    u = unknown_band(m1, band)
    return (m1.astype(np.uint8) | (u.astype(np.uint8) << 1)), m1.astype(np.uint8)


def brute_force_lift_labels(mask: np.ndarray, full_shape, band: int):
    """The same as loops over output pixels in Python floats, the edge and the band as loops over their windows."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    h1, w1 = full_shape
    m1 = np.zeros((h1, w1), bool)
    for y in range(h1):
        ya, yb, wy = _coord(y, h1, h)
        for x in range(w1):
            xa, xb, wx = _coord(x, w1, w)
            v = _lerp(_lerp(float(m[ya, xa]), float(m[ya, xb]), wx), _lerp(float(m[yb, xa]), float(m[yb, xb]), wx), wy)
            m1[y, x] = v >= 0.5
    edge = np.zeros((h1, w1), bool)
    for y in range(h1):
        for x in range(w1):
            win = m1[max(0, y - 1):y + 2, max(0, x - 1):x + 2]
            edge[y, x] = win.any() and not win.all()
    labels = np.zeros((h1, w1), np.uint8)
    for y in range(h1):
        for x in range(w1):
            u = edge[max(0, y - band):y + band + 1, max(0, x - band):x + band + 1].any()
            labels[y, x] = (3 if m1[y, x] else 2) if u else (1 if m1[y, x] else 0)
    return labels, m1.astype(np.uint8)


def chain(mask, full, band=None, n_iter: int = 1, seed: int = 0, color_space: str = "rgb",
          min_area_ratio: float = 0.002, keep_largest: bool = False, return_labels: bool = False):
    """cut_mask_full restated on the CPU oracle: -> binary (H1, W1) uint8 in {0, 1} [, labels]."""
    from oracle import oracle as orc
    full = np.ascontiguousarray(full, np.uint8)
    if band is None:
        band = default_band(np.asarray(mask).shape, full.shape[:2])
    labels, _ = lift_labels(mask, full.shape[:2], band)
    img = full if color_space == "rgb" else orc.convert_color8(full, color_space)
    binary = orc.grabcut(img, labels, n_iter=n_iter, mode=0, seed=seed)[0]
    out = orc.clean_mask(binary, min_area_ratio, keep_largest)
    return (out, labels) if return_labels else out


# ---------------------------------------------------------------- the scenes of the study and of the quality tests
def box_down(a: np.ndarray, k: int) -> np.ndarray:
    """(H, W[, C]) -> (H / k, W / k[, C]) float64 means of the k x k boxes (H, W multiples of k)."""
    a = np.asarray(a, np.float64)
    h, w = a.shape[0] // k, a.shape[1] // k
    return a.reshape(h, k, w, k, *a.shape[2:]).mean(axis=(1, 3))


def scene(h1: int, w1: int, seed: int, k: int = 4):
    """-> (full bgr u8 (h1, w1, 3), truth u8 (h1, w1), working bgr u8 = the rounded k x k box mean)."""
    from gcn_grabcut.synthetic import synthetic_image
    full, truth = synthetic_image(h1, w1, seed, return_mask=True)
    return full, (truth != 0).astype(np.uint8), np.rint(box_down(full, k)).astype(np.uint8)


def working_masks(truth: np.ndarray, k: int = 4):
    """-> (good, shifted): the box mean of the truth >= 0.5, and that rolled by one working pixel to the right (a stand-in
    for a segmentation error)."""
    good = (box_down(truth, k) >= 0.5).astype(np.uint8)
    return good, np.roll(good, 1, axis=1)


GUIDED = (8, 1e-4)          # radius, eps of the guided upsample the study compares with


def guided_mask(work: np.ndarray, mask: np.ndarray, full: np.ndarray) -> np.ndarray:
    """What full.binary_mask is without full_cut: the guided upsample's alpha >= 0.5 (upsample_ref)."""
    return (upsample_ref(work, mask, full, *GUIDED) >= 0.5).astype(np.uint8)


def wrong(mask: np.ndarray, truth: np.ndarray) -> int:
    return int(np.count_nonzero((np.asarray(mask) != 0) != (np.asarray(truth) != 0)))


STUDY_SEEDS = tuple(range(30000, 30006))
STUDY_SIZE = (240, 320, 4)


def study_totals(bands=(None,), seeds=STUDY_SEEDS, size=STUDY_SIZE, cut=chain):
    """Wrong pixels against the truth summed over the scenes -> {row: (good, shifted)} with the rows "lifted", "guided"
    and ("cut", band) for every band asked for (None = the default band).  cut(mask, full, band) -> binary."""
    h1, w1, k = size
    rows = {"lifted": [0, 0], "guided": [0, 0], **{("cut", b): [0, 0] for b in bands}}
    for s in seeds:
        full, truth, work = scene(h1, w1, s, k)
        for j, m in enumerate(working_masks(truth, k)):
            rows["lifted"][j] += wrong(lift_labels(m, (h1, w1), 0)[1], truth)
            rows["guided"][j] += wrong(guided_mask(work, m, full), truth)
            for b in bands:
                rows[("cut", b)][j] += wrong(cut(m, full, b), truth)
    return {k_: tuple(v) for k_, v in rows.items()}
