"""
GCN-GrabCut end-to-end pipeline — host mirror of reference src/gcn_grabcut/pipeline.py.

  1. superpixel graph (+ automatic FG/BG prior)      ggc_preprocess, ggc_slic, ggc_graph_*
  2. ResGCNNet -> region probabilities               ggc_resgcn_forward
  3. guided-filter projection -> pixel trimap        ggc_refine_trimap (+ ggc_seed_from_prior)
  4. GrabCut refinement -> binary mask               ggc_grabcut
  5. clean-up and output composition                 ggc_clean_mask, ggc_compose_outputs

`segment(image)` keeps the reference signature and result type; `segment_batch`
(additive) runs the same stages over a batch of equally sized images with every
intermediate resident in HBM.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from .grabcut import GrabCut, GrabCutConfig, Label
from .graph_builder import (GraphBuilder, SuperpixelGraphConfig, graphs_to_host, _check_image, pack_hints, pack_strokes,
                            pack_polygons, lasso_list, pack_paths, scissors_list, POLYGON_LASSO)
from .metrics import evaluate, evaluate_matte, evaluate_trimap, MatteMetrics, SegmentationMetrics, TrimapMetrics
from .model import CLASS_BG, CLASS_FG, project_to_pixels  # noqa: F401


def _write_png(path: str, array: np.ndarray) -> None:
    """cv2.imwrite stand-in (OpenCV is not a dependency): BGR(A) array -> PNG via Pillow."""
    from PIL import Image
    a = np.asarray(array)
    if a.ndim == 3 and a.shape[2] == 3:
        a = a[:, :, ::-1]
    elif a.ndim == 3 and a.shape[2] == 4:
        a = a[:, :, [2, 1, 0, 3]]
    Image.fromarray(np.ascontiguousarray(a)).save(path)


@dataclass
class FullResolution:
    """The outputs of a run at the full resolution of the image it was given (additive; upsample_mask): (H1, W1) arrays."""
    binary_mask: np.ndarray                  # (H1, W1) uint8 {0, 1}: upsampled alpha >= 0.5 (full_cut: cut_mask_full)
    overlay: np.ndarray                      # (H1, W1, 3) BGR with coloured overlay of binary_mask
    rgba: np.ndarray                         # (H1, W1, 4) BGRA, alpha = 255 * binary_mask
    alpha: Optional[np.ndarray] = None       # (H1, W1) float32 soft matte in [0, 1] (matte=True)
    rgba_soft: Optional[np.ndarray] = None   # (H1, W1, 4) uint8 BGRA cut-out with alpha = round(255 alpha) (matte=True)


@dataclass
class SegmentationResult:
    """All outputs from one pipeline run (reference pipeline.py:32-68)."""
    image: np.ndarray          # original BGR
    binary_mask: np.ndarray    # (H, W) uint8 {0, 1}
    trimap: np.ndarray         # (H, W) uint8 {0,1,2,3}
    segments: np.ndarray       # (H, W) superpixel map
    overlay: np.ndarray        # BGR with coloured overlay
    rgba: np.ndarray           # BGRA transparent background
    timing: dict = field(default_factory=dict)
    alpha: Optional[np.ndarray] = None       # additive: (H, W) float32 soft matte in [0, 1] (matte=True)
    rgba_soft: Optional[np.ndarray] = None   # additive: (H, W, 4) uint8 BGRA cut-out with alpha = round(255 alpha)
    full: Optional[FullResolution] = None    # additive: the outputs at the full image's resolution (full_image=...)
    foreground: Optional[np.ndarray] = None  # additive: (H, W, 3) uint8 BGR estimated foreground colours (foreground=True)
    rgba_clean: Optional[np.ndarray] = None  # additive: (H, W, 4) uint8 BGRA cut-out of `foreground`, alpha = round(255 alpha)

    def save(self, prefix: str = "result") -> None:
        _write_png(f"{prefix}_overlay.png", self.overlay)
        _write_png(f"{prefix}_rgba.png", self.rgba)
        _write_png(f"{prefix}_trimap_colour.png", _colour_trimap(self.trimap))
        _write_png(f"{prefix}_mask.png", self.binary_mask * 255)
        if self.alpha is not None:
            _write_png(f"{prefix}_alpha.png", alpha_to_u8(self.alpha))
        if self.rgba_soft is not None:
            _write_png(f"{prefix}_cutout.png", self.rgba_soft)
        if self.rgba_clean is not None:
            _write_png(f"{prefix}_cutout_clean.png", self.rgba_clean)
        if self.full is not None:
            f = self.full
            _write_png(f"{prefix}_full_mask.png", f.binary_mask * 255)
            _write_png(f"{prefix}_full_overlay.png", f.overlay)
            _write_png(f"{prefix}_full_rgba.png", f.rgba)
            if f.alpha is not None:
                _write_png(f"{prefix}_full_alpha.png", alpha_to_u8(f.alpha))
            if f.rgba_soft is not None:
                _write_png(f"{prefix}_full_cutout.png", f.rgba_soft)
        print(f"Saved outputs with prefix: {prefix}")

    def evaluate_against(self, gt_mask: np.ndarray) -> "tuple[SegmentationMetrics, TrimapMetrics]":
        """Segmentation and trimap metrics against a ground-truth mask (reference pipeline.py:62-68)."""
        return evaluate(self.binary_mask, gt_mask), evaluate_trimap(self.trimap, gt_mask)

    def evaluate_matte_against(self, gt_alpha: np.ndarray, region: Optional[np.ndarray] = None) -> "MatteMetrics":
        """SAD, MSE, gradient and connectivity error of this result's matte against the true matte (additive;
        metrics.evaluate_matte).  gt_alpha: (H, W) uint8 levels or floats in [0, 1]; region: nonzero = counted."""
        if self.alpha is None:
            raise ValueError("this result carries no matte: segment with matte=True or a ClosedFormMatte")
        return evaluate_matte(self.alpha, gt_alpha, region)

    def outlines(self, connectivity: int = 8, full: bool = False) -> "list[Outline]":
        """The exact vector outlines of binary_mask, or of full.binary_mask with full=True (additive; mask_outlines)."""
        if full and self.full is None:
            raise ValueError("this result carries no full-resolution outputs: segment with full_image=...")
        return mask_outlines(self.full.binary_mask if full else self.binary_mask, connectivity)

    def modified(self, *steps: "ModifyMask", full: bool = False) -> np.ndarray:
        """binary_mask, or full.binary_mask with full=True, after the steps in order (additive; modify_mask)."""
        if full and self.full is None:
            raise ValueError("this result carries no full-resolution outputs: segment with full_image=...")
        return modify_mask(self.full.binary_mask if full else self.binary_mask, *steps)

    def trimap_from_mask(self, inner, outer=None, full: bool = False) -> np.ndarray:
        """A 0 / 128 / 255 trimap for trimap_matte with an unknown band of the given radii around the mask's boundary
        (additive; mask_to_trimap)."""
        return self.modified(ModifyMask("trimap", inner, outer), full=full)

    def composite_onto(self, background: np.ndarray, offset=(0, 0), method: str = "over", full: bool = False) -> np.ndarray:
        """This result placed on background (H, W, 3) uint8 BGR with its pixel (0, 0) at offset = (row, col) (additive).
        method "over": alpha-over of the cleanest cut-out the result carries, rgba_clean, else rgba_soft, else rgba
        (composite_over); "seamless" | "mixed": the image under binary_mask cloned in the gradient domain with the
        source's or with mixed gradients (seamless_clone).  full=True uses result.full's members.  -> (H, W, 3) uint8 BGR."""
        if method not in ("over", "seamless", "mixed"):
            raise ValueError(f"composite_onto: method must be 'over', 'seamless' or 'mixed', got {method!r}")
        if full and self.full is None:
            raise ValueError("this result carries no full-resolution outputs: segment with full_image=...")
        r = self.full if full else self
        if method == "over":
            clean = None if full else self.rgba_clean
            return composite_over(clean if clean is not None else r.rgba_soft if r.rgba_soft is not None else r.rgba,
                                  background, offset)
        image = r.rgba[..., :3] if full else self.image          # the full-size cut-out keeps the full image's bytes
        return seamless_clone(np.ascontiguousarray(image), r.binary_mask, background, offset, mixed=method == "mixed")


def guided_filter(guide: np.ndarray, src: np.ndarray, radius: int = 8, eps: float = 1e-3, device="cuda") -> np.ndarray:
    """Edge-preserving filter of `src` under `guide` (He et al.) — reference pipeline.py:71-100."""
    from ._engine import get_engine
    eng = get_engine(device)
    g = eng.to_device(np.ascontiguousarray(guide, dtype=np.float32)[None])
    s = eng.to_device(np.ascontiguousarray(src, dtype=np.float32)[None])
    return eng.guided_filter(g, s, radius, eps)[0].cpu().numpy()


MATTE_RADIUS = 4
MATTE_EPS = 1e-4


def _check_mask(mask, what: str, shape=None) -> np.ndarray:
    """`what`'s mask as an array: values in {0, 1}, and (H, W) = shape when that is given."""
    m = np.asarray(mask)
    if shape is not None and m.shape != shape:
        raise ValueError(f"{what}: mask {m.shape} does not match image {shape}")
    if m.size and not np.isin(m, (0, 1)).all():
        raise ValueError(f"{what}: mask values must be 0 or 1")
    return m


def _check_trimap(trimap, what: str, shape) -> np.ndarray:
    """`what`'s trimap as an array: (H, W) = shape, uint8."""
    t = np.asarray(trimap)
    if t.shape != shape:
        raise ValueError(f"{what}: trimap {t.shape} does not match image {shape}")
    if t.dtype != np.uint8:
        raise ValueError(f"{what}: trimap must be uint8 (255 foreground, 0 background, else unknown), got {t.dtype}")
    return t


def _with_info(value, iters, rel, return_info: bool):
    """A solver's host result for one image: with return_info, (value, iterations, relative residual)."""
    return (value, int(iters[0].item()), float(rel[0].item())) if return_info else value


def alpha_to_u8(alpha: np.ndarray) -> np.ndarray:
    """(H, W) alpha in [0, 1] -> uint8 round(255 alpha), the alpha channel of a cut-out."""
    return np.floor(np.asarray(alpha, np.float64) * 255.0 + 0.5).astype(np.uint8)


def alpha_matte(image: np.ndarray, mask: np.ndarray, radius: int = MATTE_RADIUS, eps: float = MATTE_EPS,
                device="cuda") -> np.ndarray:
    """Soft alpha matte of a binary mask (additive): He, Sun and Tang's guided filter with the colour image as guide
    (I = bgr / 255, a 3x3 covariance per window) and the mask as input, clamped to [0, 1] (ggc_alpha_matte).  Pixels
    farther than 2 * radius from the mask's edge keep the mask's value exactly; near it, alpha follows the colours.

    image: (H, W, 3) uint8 BGR; mask: (H, W) with values in {0, 1} (bool or integer).  radius in 1..64, eps >= 1e-12.
    The defaults (radius 4, eps 1e-4, for images whose longest side is about 800 pixels, inference.py's --max-size) are
    a choice, not a tuned result.
    -> (H, W) float32."""
    from ._engine import get_engine, check_matte_args
    image = _check_image(image)
    m = _check_mask(mask, "alpha_matte", image.shape[:2])
    check_matte_args(radius, eps)
    eng = get_engine(device)
    bgr = eng.to_device(image[None])
    binary = eng.to_device(np.ascontiguousarray(m, dtype=np.uint8)[None])
    return eng.alpha_matte(bgr, binary, radius, eps)[0].cpu().numpy()


CF_RADIUS = 1
CF_EPS = 1e-5
CF_BAND = 1
CF_MAX_ITER = 500
CF_TOL = 1e-4
CF_FULL_MAX_ITER = 2000      # the iteration limit of the full-size solve: a recorded choice, not a tuned one
CF_GROW = 0


@dataclass(frozen=True)
class ClosedFormMatte:
    """matte=ClosedFormMatte(...) asks segment / segment_batch / segment_batch_device / segment_bbox for the closed-form
    matte (closed_form_matte) of the cleaned mask instead of the guided one (matte=True).  The defaults are a recorded
    choice from a float64 CPU study (tools/closed_form_study.py), not a tuned result.

    full_resolution=True (with a full image: full_image / full_images / full_bgr) also solves at the full image's size
    (closed_form_matte_full with grow and full_max_iter) and fills the result's full alpha, rgba_soft
    and binary_mask (alpha >= 0.5) from that.  Without it a full image is refused, as before."""
    radius: int = CF_RADIUS
    eps: float = CF_EPS
    band: int = CF_BAND
    max_iter: int = CF_MAX_ITER
    tol: float = CF_TOL
    full_resolution: bool = False
    grow: int = CF_GROW
    full_max_iter: int = CF_FULL_MAX_ITER

    def args(self) -> "tuple[int, float, int, int, float]":
        return int(self.radius), float(self.eps), int(self.band), int(self.max_iter), float(self.tol)


def closed_form_matte(image: np.ndarray, mask: np.ndarray, radius: int = CF_RADIUS, eps: float = CF_EPS,
                      band: int = CF_BAND, max_iter: int = CF_MAX_ITER, tol: float = CF_TOL, return_info: bool = False,
                      device="cuda"):
    """Closed-form alpha matte of a binary mask (additive): Levin, Lischinski and Weiss's matting Laplacian (colour-line
    model, windows of (2 radius + 1)^2 pixels wholly inside the image, regulariser eps / n) minimised over the pixels
    within `band` of the mask's edge, every other pixel held at the mask's value (ggc_closed_form_matte).  Solved by
    Jacobi-preconditioned conjugate gradients on the device until the residual falls to tol times its start, or for
    max_iter iterations.  Unlike alpha_matte it can give fractional alpha that the mask got wrong (thin strands).

    image: (H, W, 3) uint8 BGR; mask: (H, W) with values in {0, 1}.  radius in 1..8 with H, W >= 2 radius + 1,
    1e-12 <= eps <= 1, band in 0..64, max_iter in 1..100000, 1e-12 <= tol < 1.  The defaults are a recorded choice
    (DESIGN.md §5.13), not a tuned result.
    -> (H, W) float32 in [0, 1]; with return_info, (alpha, iterations, relative residual)."""
    from ._engine import get_engine, check_closed_form_args, check_closed_form_shape
    image = _check_image(image)
    m = _check_mask(mask, "closed_form_matte", image.shape[:2])
    check_closed_form_args(radius, eps, band, max_iter, tol)
    check_closed_form_shape(*image.shape[:2], radius)
    eng = get_engine(device)
    alpha, iters, rel = eng.closed_form_matte(eng.to_device(image[None]), eng.to_device(np.ascontiguousarray(m, np.uint8)[None]),
                                              radius, eps, band, max_iter, tol)
    return _with_info(alpha[0].cpu().numpy(), iters, rel, return_info)


def trimap_matte(image: np.ndarray, trimap: np.ndarray, radius: int = CF_RADIUS, eps: float = CF_EPS,
                 max_iter: int = CF_MAX_ITER, tol: float = CF_TOL, alpha0: "Optional[np.ndarray]" = None,
                 return_info: bool = False, device="cuda"):
    """Closed-form alpha matte from an image and a trimap (additive): the matting Laplacian of closed_form_matte
    minimised over the trimap's unknown pixels, with alpha 1 on its foreground and 0 on its background
    (ggc_trimap_matte).  Where closed_form_matte can only look within `band` of a mask's edge, with a
    mask that is wrong exactly there as its anchor, here the caller says where the hair is.  A tight trimap helps; a loose
    one leaves Levin's energy free to smooth fine structure away.

    image: (H, W, 3) uint8 BGR; trimap: (H, W) uint8, 255 = foreground, 0 = background, every other byte unknown (the
    convention of the matting benchmarks and of evaluate_matte.py --trimaps).  alpha0: (H, W) float, finite, or None:
    where the unknown pixels start (clamped to [0, 1]; 0.5 without it); it changes the iterations, and the answer within
    tol.  radius, eps, max_iter and tol as closed_form_matte.  A trimap without unknown pixels, or with nothing else,
    returns the start.  trimap_matte_warm is the same solve with a stop rule made for a good alpha0.
    -> (H, W) float32 in [0, 1]; with return_info, (alpha, iterations, relative residual)."""
    return _trimap_matte(image, trimap, radius, eps, max_iter, tol, alpha0, return_info, device, False)


def trimap_matte_warm(image: np.ndarray, trimap: np.ndarray, alpha0: np.ndarray, radius: int = CF_RADIUS,
                      eps: float = CF_EPS, max_iter: int = CF_MAX_ITER, tol: float = CF_TOL, return_info: bool = False,
                      device="cuda"):
    """trimap_matte from a start that is already close (additive; ggc_trimap_matte_warm): the solve stops
    when the residual falls to tol times that of the 0.5 start, not of alpha0's own, so a good alpha0 saves iterations
    (none at all when it is already within tol), and the relative residual returned is relative to that too.  With
    alpha0 = 0.5 it is trimap_matte(alpha0=None) bit for bit.  alpha0 is required (None is a ValueError); every other
    argument as trimap_matte.  It is a function of its own because trimap_matte's parameter list is pinned.
    -> (H, W) float32 in [0, 1]; with return_info, (alpha, iterations, relative residual)."""
    if alpha0 is None:
        raise ValueError("trimap_matte_warm needs alpha0, the start it is warm from")
    return _trimap_matte(image, trimap, radius, eps, max_iter, tol, alpha0, return_info, device, True)


def _trimap_matte(image, trimap, radius, eps, max_iter, tol, alpha0, return_info, device, warm):
    """trimap_matte and trimap_matte_warm: the checks, then Engine.trimap_matte on a batch of one."""
    from ._engine import get_engine, check_closed_form_args, check_closed_form_shape
    image = _check_image(image)
    t = _check_trimap(trimap, "trimap_matte", image.shape[:2])
    a0 = None
    if alpha0 is not None:
        a0 = np.asarray(alpha0)
        if a0.shape != image.shape[:2]:
            raise ValueError(f"trimap_matte: alpha0 {a0.shape} does not match image {image.shape[:2]}")
        if a0.dtype.kind != "f":
            raise ValueError(f"trimap_matte: alpha0 must be a float array, got {a0.dtype}")
        if not np.isfinite(a0).all():
            raise ValueError("trimap_matte: alpha0 must be finite")
    check_closed_form_args(radius, eps, 0, max_iter, tol)
    check_closed_form_shape(*image.shape[:2], radius)
    eng = get_engine(device)
    start = None if a0 is None else eng.to_device(np.ascontiguousarray(a0, np.float32)[None])
    alpha, iters, rel = eng.trimap_matte(eng.to_device(image[None]), eng.to_device(np.ascontiguousarray(t)[None]), radius,
                                         eps, max_iter, tol, alpha0=start, warm=warm)
    return _with_info(alpha[0].cpu().numpy(), iters, rel, return_info)


def lift_trimap(trimap: np.ndarray, alpha: np.ndarray, full_shape, grow: int = CF_GROW, device="cuda"):
    """A working-size trimap and alpha carried to a larger size (additive; ggc_lift_trimap): the trimap
    and the start of a closed-form solve on the full image.  Every output pixel looks at the source pixels bilinear
    interpolation (half-pixel centres, as upsample_mask) gives it a nonzero weight for: it is foreground (255) or
    background (0) when all of them are, else unknown (128); the unknown region is then dilated by `grow` full-size
    pixels.  The start is the bilinear interpolation of alpha clamped to [0, 1].

    trimap: (H, W) uint8, 255 = foreground, 0 = background, every other byte unknown; alpha: (H, W) float, finite;
    full_shape: (H1, W1) with H <= H1 <= 32768, W <= W1 <= 32768; grow in 0..64.
    -> (trimap_full (H1, W1) uint8, alpha0_full (H1, W1) float32)."""
    from ._engine import get_engine, check_lift_args
    t, a = np.asarray(trimap), np.asarray(alpha)
    if t.ndim != 2 or t.dtype != np.uint8:
        raise ValueError(f"lift_trimap: trimap must be (H, W) uint8, got {t.shape} {t.dtype}")
    if a.dtype.kind != "f":
        raise ValueError(f"lift_trimap: alpha must be a float array, got {a.dtype}")
    full_shape = tuple(int(v) for v in full_shape)
    check_lift_args((1, *t.shape), (1, *a.shape), full_shape, grow)
    if not np.isfinite(a).all():
        raise ValueError("lift_trimap: alpha must be finite")
    eng = get_engine(device)
    t_full, a_full = eng.lift_trimap(eng.to_device(np.ascontiguousarray(t)[None]),
                                     eng.to_device(np.ascontiguousarray(a, np.float32)[None]), full_shape, grow)
    return t_full[0].cpu().numpy(), a_full[0].cpu().numpy()


def _check_full_solve(image, full_image, radius, eps, band, max_iter, tol, grow, full_max_iter, what):
    """The arguments the two full-resolution chains share, checked before any device call -> (image, full_image)."""
    from ._engine import check_closed_form_args, check_closed_form_shape, check_lift_args
    image, full = _check_image(image), _check_image(full_image)
    check_closed_form_args(radius, eps, band, max_iter, tol)
    check_closed_form_args(radius, eps, band, full_max_iter, tol)
    check_closed_form_shape(*image.shape[:2], radius)
    try:
        check_lift_args((1, *image.shape[:2]), None, full.shape[:2], grow)
    except ValueError as e:
        raise ValueError(str(e).replace("lift_trimap", what)) from None
    return image, full


def _full_solve_result(eng, bgr_full, trimap, alpha, radius, eps, grow, full_max_iter, tol, return_info):
    a_full, _, iters, rel = eng.closed_form_full(bgr_full, trimap, alpha, bgr_full, radius, eps, grow, full_max_iter, tol)
    return _with_info(a_full[0].cpu().numpy(), iters, rel, return_info)


def closed_form_matte_full(image: np.ndarray, mask: np.ndarray, full_image: np.ndarray, radius: int = CF_RADIUS,
                           eps: float = CF_EPS, band: int = CF_BAND, max_iter: int = CF_MAX_ITER, tol: float = CF_TOL,
                           grow: int = CF_GROW, full_max_iter: int = CF_FULL_MAX_ITER, return_info: bool = False,
                           device="cuda"):
    """The closed-form matte of a working-size mask, solved again on the full-resolution image (additive; DESIGN.md
    §5.17).  Four steps, all on the device: closed_form_matte(image, mask, radius, eps, band, max_iter, tol); the band
    that solve ran on written as a trimap (128 on the band, else 255 mask; ggc_closed_form_band); that trimap and the
    solved alpha lifted to full_image's size (lift_trimap with grow); and the warm solve there
    (trimap_matte_warm(full_image, lifted trimap, lifted alpha, max_iter=full_max_iter)), which sees the
    full image's colours where upsample_mask can only interpolate coefficients.

    image: (H, W, 3) uint8 BGR; mask: (H, W) in {0, 1}; full_image: (H1, W1, 3) uint8 BGR, H <= H1 <= 32768 and
    W <= W1 <= 32768; grow in 0..64 (0: growing the lifted region did not help in the study); full_max_iter in
    1..100000 (an image that reaches it reports it in the iterations).
    -> (H1, W1) float32 in [0, 1]; with return_info, (alpha, iterations, relative residual) of the full-size solve."""
    from ._engine import get_engine
    image, full = _check_full_solve(image, full_image, radius, eps, band, max_iter, tol, grow, full_max_iter,
                                    "closed_form_matte_full")
    m = _check_mask(mask, "closed_form_matte_full", image.shape[:2])
    eng = get_engine(device)
    binary = eng.to_device(np.ascontiguousarray(m, np.uint8)[None])
    alpha, _, _ = eng.closed_form_matte(eng.to_device(image[None]), binary, radius, eps, band, max_iter, tol)
    return _full_solve_result(eng, eng.to_device(full[None]), eng.closed_form_band(binary, band), alpha, radius, eps, grow,
                              full_max_iter, tol, return_info)


def trimap_matte_full(image: np.ndarray, trimap: np.ndarray, full_image: np.ndarray, radius: int = CF_RADIUS,
                      eps: float = CF_EPS, max_iter: int = CF_MAX_ITER, tol: float = CF_TOL, grow: int = CF_GROW,
                      full_max_iter: int = CF_FULL_MAX_ITER, return_info: bool = False, device="cuda"):
    """closed_form_matte_full from a caller's working-size trimap (additive): trimap_matte(image, trimap) at the working
    size, that trimap and alpha lifted to full_image's size (lift_trimap with grow), and the warm solve there.

    trimap: (H, W) uint8, 255 = foreground, 0 = background, every other byte unknown; the rest as
    closed_form_matte_full.
    -> (H1, W1) float32 in [0, 1]; with return_info, (alpha, iterations, relative residual) of the full-size solve."""
    from ._engine import get_engine
    image, full = _check_full_solve(image, full_image, radius, eps, 0, max_iter, tol, grow, full_max_iter,
                                    "trimap_matte_full")
    t = _check_trimap(trimap, "trimap_matte_full", image.shape[:2])
    eng = get_engine(device)
    tri = eng.to_device(np.ascontiguousarray(t)[None])
    alpha, _, _ = eng.trimap_matte(eng.to_device(image[None]), tri, radius, eps, max_iter, tol)
    return _full_solve_result(eng, eng.to_device(full[None]), tri, alpha, radius, eps, grow, full_max_iter, tol, return_info)


FG_EPS_R = 5e-3
FG_OMEGA = 1.0
FG_MAX_ITER = 2000
FG_TOL = 1e-6


@dataclass(frozen=True)
class ForegroundColours:
    """foreground=ForegroundColours(...) (or foreground=True for the defaults) asks segment / segment_batch /
    segment_batch_device / segment_bbox, together with a matte, for the estimated foreground colours under that matte
    (estimate_foreground): result.foreground and the clean cut-out result.rgba_clean.  The defaults are a recorded choice
    from a float64 CPU study (tools/foreground_study.py), not a tuned result."""
    eps_r: float = FG_EPS_R
    omega: float = FG_OMEGA
    max_iter: int = FG_MAX_ITER
    tol: float = FG_TOL

    def args(self) -> "tuple[float, float, int, float]":
        return float(self.eps_r), float(self.omega), int(self.max_iter), float(self.tol)


def estimate_foreground(image: np.ndarray, alpha: np.ndarray, eps_r: float = FG_EPS_R, omega: float = FG_OMEGA,
                        max_iter: int = FG_MAX_ITER, tol: float = FG_TOL, return_info: bool = False, device="cuda"):
    """Foreground colours under an alpha matte (additive): where alpha is fractional the image's colour is the blend
    alpha F + (1 - alpha) B, and a cut-out that keeps it shows a halo of the old background on a new one.  This solves
    for F (and B) on those pixels: Germer, Uelwer, Conrad and Harmeling's foreground estimation energy (the blend
    equation plus smoothness of F and B, weaker across changes of alpha: weight eps_r + omega |alpha_i - alpha_j|) with
    the pixels of alpha 0 and 1 held at the image's colour, by preconditioned conjugate gradients on the device until the
    residual falls to tol times its start, or for max_iter iterations (ggc_estimate_foreground).

    image: (H, W, 3) uint8 BGR; alpha: (H, W) float in [0, 1] (alpha_matte's or closed_form_matte's output; values whose
    byte round(255 alpha) is 0 or 255 count as 0 and 1; a NaN counts as 0).  0 <= eps_r <= 1, 0 <= omega <= 1000, not
    both 0, max_iter in 1..100000, 1e-12 <= tol < 1.
    -> (H, W, 3) uint8 BGR: F where alpha is fractional, the image elsewhere; with return_info, (foreground, iterations,
    relative residual)."""
    from ._engine import get_engine, check_foreground_args
    image = _check_image(image)
    a = np.asarray(alpha)
    if a.shape != image.shape[:2]:
        raise ValueError(f"estimate_foreground: alpha {a.shape} does not match image {image.shape[:2]}")
    if a.dtype.kind != "f":
        raise ValueError(f"estimate_foreground: alpha must be a float array, got {a.dtype}")
    check_foreground_args(eps_r, omega, max_iter, tol)
    eng = get_engine(device)
    fg, iters, rel = eng.estimate_foreground(eng.to_device(image[None]),
                                             eng.to_device(np.ascontiguousarray(a, np.float32)[None]), eps_r, omega,
                                             max_iter, tol)
    return _with_info(fg[0].cpu().numpy(), iters, rel, return_info)


CLONE_MAX_ITER = 10000
CLONE_TOL = 1e-7


@dataclass(frozen=True)
class Clone:
    """The options of seamless cloning (ggc_poisson_clone, include/ggc.h O6).  mixed=False keeps the
    source's gradients inside the pasted region ("seamless"); mixed=True takes, per pixel pair and channel, the stronger
    of the source's and the target's gradient, so that the target's texture shows through flat parts of the source.
    The solve stops when the residual falls to tol times its start, or after max_iter iterations.  The defaults are
    recorded choices, not tuned results."""
    mixed: bool = False
    max_iter: int = CLONE_MAX_ITER
    tol: float = CLONE_TOL

    def __post_init__(self):
        from ._engine import check_clone_args
        if not isinstance(self.mixed, (bool, np.bool_)):
            raise ValueError(f"Clone: mixed must be a bool, got {self.mixed!r}")
        check_clone_args(self.mixed, self.max_iter, self.tol)

    def args(self) -> "tuple[bool, int, float]":
        return bool(self.mixed), int(self.max_iter), float(self.tol)


def _offsets(offset, b: int, what: str) -> np.ndarray:
    """One (row, col) pair for every image, or one pair per image -> (B, 2) int64."""
    try:
        off = np.asarray(offset)
    except ValueError:
        off = None
    if off is None or off.dtype.kind not in "iu" or off.shape not in ((2,), (b, 2)):
        raise ValueError(f"{what}: offset must be a (row, col) pair of integers, or one pair per image, got {offset!r}")
    return np.broadcast_to(off.astype(np.int64), (b, 2))


def _rgba_batch(cutouts, what: str) -> np.ndarray:
    """A (B, Hs, Ws, 4) uint8 array, or a sequence of equally sized (Hs, Ws, 4) uint8 BGRA cut-outs -> (B, Hs, Ws, 4)."""
    a = cutouts if isinstance(cutouts, np.ndarray) and cutouts.ndim == 4 else None
    if a is None:
        items = [np.asarray(c) for c in cutouts]
        if any(c.ndim != 3 or c.shape != items[0].shape for c in items):
            raise ValueError(f"{what} needs (Hs, Ws, 4) cut-outs of one size; group them by shape")
        a = np.stack(items) if items else np.zeros((0, 1, 1, 4), np.uint8)
    if a.dtype != np.uint8 or a.shape[3] != 4 or a.shape[1] < 1 or a.shape[2] < 1:
        raise ValueError(f"{what}: cut-outs must be (Hs, Ws, 4) uint8 BGRA, got {a.shape[1:]} {a.dtype}")
    return np.ascontiguousarray(a)


def composite_over_batch(cutouts, backgrounds, offsets=(0, 0), device="cuda") -> np.ndarray:
    """BGRA cut-outs placed on backgrounds by alpha-over (additive; ggc_composite_over).  cutouts:
    (B, Hs, Ws, 4) uint8 or a sequence of equally sized cut-outs (rgba, rgba_soft or rgba_clean of a result); backgrounds:
    (B, H, W, 3) uint8 BGR or a sequence of equally sized images; offsets: one (row, col) pair, or one per image, the
    place of the cut-out's pixel (0, 0) in the background, negative allowed, within +-32768.  Integer arithmetic:
    (a c + (255 - a) bg + 127) // 255 per channel where the cut-out covers the background, the background elsewhere.
    -> (B, H, W, 3) uint8 BGR."""
    from ._engine import check_composite_args, get_engine
    rgba = _rgba_batch(cutouts, "composite_over_batch")
    bg = _image_batch(backgrounds, "composite_over_batch")
    if len(rgba) != len(bg):
        raise ValueError(f"composite_over_batch: {len(rgba)} cut-outs for {len(bg)} backgrounds")
    off = check_composite_args(rgba.shape, bg.shape, _offsets(offsets, len(bg), "composite_over_batch"),
                               (rgba.dtype, bg.dtype), 4, "composite_over_batch")
    if len(bg) == 0:
        return bg.copy()
    eng = get_engine(device)
    return eng.composite_over(eng.to_device(rgba), eng.to_device(bg), off).cpu().numpy()


def composite_over(rgba: np.ndarray, background: np.ndarray, offset=(0, 0), device="cuda") -> np.ndarray:
    """One (Hs, Ws, 4) uint8 BGRA cut-out placed on an (H, W, 3) uint8 BGR background with its pixel (0, 0) at offset =
    (row, col) (additive; composite_over_batch).  -> (H, W, 3) uint8 BGR."""
    c = np.asarray(rgba)
    if c.ndim != 3:
        raise ValueError(f"composite_over: the cut-out must be (Hs, Ws, 4) uint8 BGRA, got {c.shape}")
    return composite_over_batch(c[None], _check_image(background)[None], offset, device)[0]


def seamless_clone_batch(sources, masks, targets, offsets=(0, 0), clone: Optional[Clone] = None, return_info: bool = False,
                         device="cuda"):
    """Seamless (Poisson) cloning of a batch (additive; ggc_poisson_clone).  sources: (B, Hs, Ws, 3)
    uint8 BGR or a sequence of equally sized images; masks: (B, Hs, Ws), non-zero = selected; targets: (B, H, W, 3) uint8
    BGR or a sequence of equally sized images; offsets as composite_over_batch's.  Inside the selection the result has
    the source's gradients (or, with Clone(mixed=True), the stronger of the source's and the target's) and meets the
    target's colours at its boundary; outside it is the target.
    -> (B, H, W, 3) uint8 BGR; with return_info also (n_omega, iterations, relative residual), (B,) arrays."""
    from ._engine import check_composite_args, get_engine
    if clone is None:
        clone = Clone()
    if not isinstance(clone, Clone):
        raise ValueError(f"clone must be a Clone or None, got {type(clone).__name__}")
    src = _image_batch(sources, "seamless_clone_batch")
    tgt = _image_batch(targets, "seamless_clone_batch")
    m = masks if isinstance(masks, np.ndarray) else (np.stack([np.asarray(x) for x in masks]) if len(masks) else
                                                     np.zeros((0, 1, 1), np.uint8))
    if m.shape != src.shape[:3]:
        raise ValueError(f"seamless_clone_batch: masks {m.shape} do not match the sources {src.shape[:3]}")
    if m.dtype.kind not in "biu":
        raise ValueError(f"seamless_clone_batch: masks must be bool or integer arrays (non-zero = selected), got {m.dtype}")
    if len(src) != len(tgt):
        raise ValueError(f"seamless_clone_batch: {len(src)} sources for {len(tgt)} targets")
    off = check_composite_args(src.shape, tgt.shape, _offsets(offsets, len(tgt), "seamless_clone_batch"),
                               (src.dtype, tgt.dtype), 3, "seamless_clone_batch")
    if len(tgt) == 0:
        z = np.zeros(0, np.int32)
        return (tgt.copy(), z, z, np.zeros(0)) if return_info else tgt.copy()
    eng = get_engine(device)
    comp, n, it, rel = eng.poisson_clone(eng.to_device(src), eng.to_device(np.ascontiguousarray(m != 0).view(np.uint8)),
                                         eng.to_device(tgt), off, *clone.args())
    comp = comp.cpu().numpy()
    return (comp, n.cpu().numpy(), it.cpu().numpy(), rel.cpu().numpy()) if return_info else comp


def seamless_clone(source: np.ndarray, mask: np.ndarray, target: np.ndarray, offset=(0, 0), mixed: bool = False,
                   max_iter: int = CLONE_MAX_ITER, tol: float = CLONE_TOL, return_info: bool = False, device="cuda"):
    """Seamless (Poisson) cloning of one image (additive; seamless_clone_batch): the pixels of source (Hs, Ws, 3) uint8
    BGR selected by mask (Hs, Ws), non-zero = selected, cloned into target (H, W, 3) uint8 BGR with the source's pixel
    (0, 0) at offset = (row, col).  mixed=True uses mixed gradients.
    -> (H, W, 3) uint8 BGR; with return_info, (composite, |Omega|, iterations, relative residual)."""
    out = seamless_clone_batch(_check_image(source)[None], np.asarray(mask)[None], _check_image(target)[None], offset,
                               Clone(mixed, max_iter, tol), return_info, device)
    return (out[0][0], int(out[1][0]), int(out[2][0]), float(out[3][0])) if return_info else out[0]


def upsample_mask(image: np.ndarray, mask: np.ndarray, full_image: np.ndarray, radius: int = MATTE_RADIUS,
                  eps: float = MATTE_EPS, device="cuda") -> "tuple[np.ndarray, np.ndarray]":
    """A mask found on a reduced image, carried to the full-resolution image (additive): He and Sun's fast guided filter.
    The guided filter's coefficients of alpha_matte(image, mask, radius, eps) are interpolated bilinearly (half-pixel
    centres, as cv2.resize INTER_LINEAR) to full_image's size and applied to its colours, so edges follow the full image
    (ggc_upsample_matte).  With full_image == image the alpha is alpha_matte's, bit for bit.

    image: (H, W, 3) uint8 BGR; mask: (H, W) with values in {0, 1}; full_image: (H1, W1, 3) uint8 BGR with H1 >= H and
    W1 >= W (at most 32768 on a side).  -> (alpha (H1, W1) float32 in [0, 1], mask (H1, W1) uint8 = alpha >= 0.5)."""
    from ._engine import get_engine, check_matte_args, check_upsample_shapes
    image = _check_image(image)
    full = _check_image(full_image)
    m = np.asarray(mask)
    check_upsample_shapes((1, *image.shape), (1, *m.shape), (1, *full.shape), "upsample_mask")
    _check_mask(m, "upsample_mask")
    check_matte_args(radius, eps)
    eng = get_engine(device)
    alpha, binary, _ = eng.upsample_matte(eng.to_device(image[None]), eng.to_device(np.ascontiguousarray(m, np.uint8)[None]),
                                          eng.to_device(full[None]), radius, eps)
    return alpha[0].cpu().numpy(), binary[0].cpu().numpy()


FULL_CUT_ITERS = 1
# The most pixels one ggc_grabcut call of the full-resolution cut is given: a batch of full images goes through it in
# sub-batches of at most this many (at least one image).  ggc_grabcut's arena is 66 bytes per pixel,
# so this is about 2.2 GB per context.  Read when a call runs, so a test can override it; results do not depend on it.
FULL_CUT_PIXELS = 1 << 25


@dataclass(frozen=True)
class FullCut:
    """full_cut=FullCut(...) (or full_cut=True for the defaults) asks segment / segment_batch / segment_batch_device /
    segment_bbox, together with a full image, for the full-size binary mask of cut_mask_full (a banded graph cut on the
    full image's own pixels) instead of the guided upsample's alpha >= 0.5.  band=None: one and a half
    working pixels, min(64, max(1, ceil(1.5 max(H1 / H, W1 / W)))), a choice backed by §5.18's table, not a tuned result."""
    band: Optional[int] = None
    n_iter: int = FULL_CUT_ITERS


@dataclass(frozen=True)
class GeodesicHints:
    """geodesic=GeodesicHints(...) (or geodesic=True for the defaults) makes a click label the pixels that are close to it
    along paths that do not cross colour edges (ggc_geodesic_hints) instead of a disk of hint_radius.
    radius in 0..16384: the reach in pixels over flat colour (limit = 80 radius); gamma in 0..64: the weight of the
    colour term; sigma > 0: the decay, in pixels, of the soft prior columns that hints_as_prior builds from the
    distances.  The defaults are recorded choices backed by §5.19's study table, not tuned results."""
    radius: int = 40
    gamma: int = 2
    sigma: float = 10.0

    def __post_init__(self):
        for name, hi in (("radius", 16384), ("gamma", 64)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= hi:
                raise ValueError(f"GeodesicHints: {name} must be an integer in [0, {hi}], got {v!r}")
        if not (isinstance(self.sigma, (int, float, np.integer, np.floating)) and np.isfinite(self.sigma) and self.sigma > 0):
            raise ValueError(f"GeodesicHints: sigma must be a positive number, got {self.sigma!r}")


def _geodesic_args(geodesic, hint_region: bool = False) -> "Optional[GeodesicHints]":
    """The GeodesicHints of a call (True: the defaults), None when the option is off; refused with hint_region."""
    if geodesic is None or geodesic is False:
        return None
    if geodesic is True:
        geodesic = GeodesicHints()
    if not isinstance(geodesic, GeodesicHints):
        raise ValueError(f"geodesic must be True, False or a GeodesicHints, got {type(geodesic).__name__}")
    if hint_region:
        raise ValueError("geodesic hints cannot be combined with hint_region=True: the superpixel pass belongs to the disks")
    return geodesic


def geodesic_hints(image: np.ndarray, fg_points, bg_points, radius: int = 40, gamma: int = 2, mask=None,
                   return_dist: bool = False, device="cuda"):
    """Geodesic click hints of one image (additive; ggc_geodesic_hints).  image: (H, W, 3) uint8 BGR;
    fg_points / bg_points: (row, col) pairs as encode_user_hints takes them.  A pixel becomes definite foreground (1) /
    background (0) when its geodesic distance to the nearest click of that label is at most 80 radius and smaller than
    the distance to any click of the other label; every other pixel keeps the label of `mask` ((H, W) uint8 GrabCut
    labels; None: all probable background, 2).  -> the painted (H, W) uint8 mask, or with return_dist=True the two
    (H, W) int32 maps (Df, Db), capped at 80 radius + 1."""
    import torch
    from ._engine import get_engine
    img = _check_image(image)
    g = GeodesicHints(radius, gamma)
    h, w = img.shape[:2]
    if mask is None:
        m = np.full((h, w), 2, np.uint8)
    else:
        m = np.ascontiguousarray(mask, np.uint8)
        if m.shape != (h, w):
            raise ValueError(f"geodesic_hints: mask {m.shape} does not match the image {(h, w)}")
    eng = get_engine(device)
    rows, ptr = pack_hints([(fg_points if fg_points is not None else [], bg_points if bg_points is not None else [])])
    if return_dist and len(rows) == 0:
        cap = np.full((h, w), 80 * g.radius + 1, np.int32)
        return cap, cap.copy()
    hint_rows, hint_ptr = eng.upload_hints(rows, ptr)
    bgr = eng.to_device(img[None])
    if return_dist:
        df, db = eng.empty(1, h, w, dtype=torch.int32), eng.empty(1, h, w, dtype=torch.int32)
        eng.geodesic_hints(bgr, hint_rows, hint_ptr, g.radius, g.gamma, dist_fg=df, dist_bg=db)
        return df[0].cpu().numpy(), db[0].cpu().numpy()
    md = eng.to_device(m[None])
    eng.geodesic_hints(bgr, hint_rows, hint_ptr, g.radius, g.gamma, mask=md)
    return md[0].cpu().numpy()


def _check_stroke_radius(radius, what: str = "stroke_radius") -> int:
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= 16384:
        raise ValueError(f"{what} must be an integer in [0, 16384], got {radius!r}")
    return int(radius)


def _mask_or_shape(mask_or_shape, what: str) -> np.ndarray:
    """An (H, W) uint8 label mask, or for an (H, W) shape a mask that is all probable background (2)."""
    if isinstance(mask_or_shape, (tuple, list)) and len(mask_or_shape) == 2 and all(isinstance(v, (int, np.integer)) for v in mask_or_shape):
        h, w = (int(v) for v in mask_or_shape)
        if h < 1 or w < 1:
            raise ValueError(f"{what}: bad shape {(h, w)}")
        return np.full((h, w), 2, np.uint8)
    m = np.ascontiguousarray(mask_or_shape, np.uint8)
    if m.ndim != 2 or m.size == 0:
        raise ValueError(f"{what}: the mask must be (H, W), got {m.shape}")
    return m


def paint_strokes(mask_or_shape, fg_strokes, bg_strokes, radius: int = 3, device="cuda") -> np.ndarray:
    """Brush strokes painted into a GrabCut label mask (additive; ggc_apply_strokes).  mask_or_shape: an
    (H, W) uint8 mask of GrabCut labels, or an (H, W) shape for a mask that starts all probable background (2).
    fg_strokes / bg_strokes: sequences of strokes, each a sequence of (row, col) vertices (graph_builder.pack_strokes).
    Every pixel within `radius` of a stroke becomes definite foreground (1) / background (0), background winning where
    the two overlap; radius 0 paints the centre line; vertices may lie outside the image.  -> the painted (H, W) uint8
    mask (a copy)."""
    from ._engine import get_engine
    radius = _check_stroke_radius(radius, "radius")
    m = _mask_or_shape(mask_or_shape, "paint_strokes")
    segs, ptr = pack_strokes([(fg_strokes, bg_strokes)])
    if ptr[-1] == 0:
        return m.copy()
    eng = get_engine(device)
    d_segs, d_ptr = eng.upload_strokes(segs, ptr)
    return eng.apply_strokes(eng.to_device(m[None]), d_segs, d_ptr, radius)[0].cpu().numpy()


def stroke_pixels(shape, fg_strokes, bg_strokes, device="cuda") -> np.ndarray:
    """The centre-line pixels of brush strokes inside an (H, W) image as a click list (additive; ggc_stroke_pixels):
    -> (P, 3) int32 rows (row, col, label 1 | 0) in raster order, each pixel once with the label of the last stroke
    segment whose centre line holds it (background strokes come after foreground ones)."""
    from ._engine import get_engine
    h, w = (int(v) for v in shape)
    if h < 1 or w < 1:
        raise ValueError(f"stroke_pixels: bad shape {(h, w)}")
    segs, ptr = pack_strokes([(fg_strokes, bg_strokes)])
    if ptr[-1] == 0:
        return np.zeros((0, 3), np.int32)
    eng = get_engine(device)
    d_segs, d_ptr = eng.upload_strokes(segs, ptr)
    return eng.stroke_pixels((1, h, w), d_segs, d_ptr)[0].cpu().numpy()


def paint_polygons(mask_or_shape, fg_polygons=(), bg_polygons=(), lasso=None, device="cuda") -> np.ndarray:
    """Filled polygons and lassos painted into a GrabCut label mask (additive; ggc_apply_polygons).
    mask_or_shape: an (H, W) uint8 mask of GrabCut labels, or an (H, W) shape for a mask that starts all probable
    background (2).  fg_polygons / bg_polygons: sequences of polygons, each a sequence of n >= 3 (row, col) vertices,
    closed implicitly; lasso: one polygon or a sequence of them.  First every pixel outside all lassos (if any is given)
    becomes definite background (0); then every pixel a fill covers becomes definite foreground (1) / background (0),
    background winning where the two overlap.  Covered is the even-odd rule with the boundary included; vertices may lie
    outside the image.  -> the painted (H, W) uint8 mask (a copy)."""
    from ._engine import get_engine
    m = _mask_or_shape(mask_or_shape, "paint_polygons")
    packed = pack_polygons([(fg_polygons, bg_polygons, lasso_list(lasso))])
    if len(packed[2]) == 0:
        return m.copy()
    eng = get_engine(device)
    return eng.apply_polygons(eng.to_device(m[None]), *eng.upload_polygons(*packed))[0].cpu().numpy()


def polygon_mask(shape, polygon, device="cuda") -> np.ndarray:
    """The pixels of an (H, W) image that a polygon COVERS (additive; ggc_apply_polygons' rule, include/ggc.h H3: on an
    edge, or an odd crossing number) as a uint8 mask, 1 = covered."""
    h, w = (int(v) for v in shape)
    if h < 1 or w < 1:
        raise ValueError(f"polygon_mask: bad shape {(h, w)}")
    return paint_polygons(np.zeros((h, w), np.uint8), [polygon], device=device)


@dataclass(frozen=True)
class Wand:
    """The options of the magic wand (ggc_wand_select, include/ggc.h H5).  tolerance in 0..255: how far,
    in the channel that differs most, a pixel's colour may lie from the seed's; connectivity 4 or 8: the neighbours
    through which a selection spreads from its seed; contiguous=False: "select similar", every pixel within the
    tolerance wherever it lies; sample 1, 3 or 5: the side of the window around the seed whose mean is the seed's
    colour.  The defaults are recorded choices (the ones image editors ship with), not tuned results."""
    tolerance: int = 32
    connectivity: int = 8
    contiguous: bool = True
    sample: int = 1

    def __post_init__(self):
        t = self.tolerance
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= int(t) <= 255:
            raise ValueError(f"Wand: tolerance must be an integer in [0, 255], got {t!r}")
        for name, allowed in (("connectivity", (4, 8)), ("sample", (1, 3, 5))):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) not in allowed:
                raise ValueError(f"Wand: {name} must be one of {allowed}, got {v!r}")
        if not isinstance(self.contiguous, (bool, np.bool_)):
            raise ValueError(f"Wand: contiguous must be a bool, got {self.contiguous!r}")

    def args(self) -> "tuple[int, int, int]":
        """(tolerance, connectivity, sample) as ggc_wand_select takes them: connectivity 0 = not contiguous."""
        return int(self.tolerance), int(self.connectivity) if self.contiguous else 0, int(self.sample)


def _wand_args(wand) -> Wand:
    if wand is None:
        return Wand()
    if not isinstance(wand, Wand):
        raise ValueError(f"wand must be a Wand or None, got {type(wand).__name__}")
    return wand


def _image_batch(images_or_array, what: str) -> np.ndarray:
    """A (B, H, W, 3) uint8 array, or a sequence of equally sized (H, W, 3) uint8 images -> (B, H, W, 3) uint8."""
    if isinstance(images_or_array, np.ndarray) and images_or_array.ndim == 4:
        a = images_or_array
        if a.dtype != np.uint8 or a.shape[3] != 3 or a.shape[1] < 1 or a.shape[2] < 1:
            raise ValueError(f"{what}: the batch must be (B, H, W, 3) uint8, got {a.shape} {a.dtype}")
        return np.ascontiguousarray(a)
    imgs = [_check_image(im) for im in images_or_array]
    if any(im.shape != imgs[0].shape for im in imgs):
        raise ValueError(f"{what} needs images of one size; group them by shape")
    return np.stack(imgs) if imgs else np.zeros((0, 1, 1, 3), np.uint8)


def wand_select_batch(images_or_array, seeds, wand: Optional[Wand] = None, return_counts: bool = False, device="cuda"):
    """Magic-wand selections of a batch (additive; ggc_wand_select).  images_or_array: (B, H, W, 3)
    uint8 BGR, or a sequence of equally sized images; seeds: one None or (fg_points, bg_points) per image, (row, col)
    pairs, or a packed (seeds, seed_ptr) pair (graph_builder.pack_hints).  A seed selects the pixels within the wand's
    tolerance of its colour (and connected to it, if contiguous); foreground seeds add, background seeds subtract, an
    image's later seed winning where selections overlap (its background seeds come after its foreground ones).
    -> (B, H, W) uint8, 255 = selected; with return_counts=True also (B, 2) int32, the pixels decided by a foreground /
    background seed."""
    wand = _wand_args(wand)
    imgs = _image_batch(images_or_array, "wand_select_batch")
    b, h, w = imgs.shape[:3]
    rows, ptr = _host_packed(seeds if seeds is not None else [None] * b, b, "seeds", 3, pack_hints, 2,
                             lambda a: [(a[1], "seed_ptr", b, len(a[0]), 0)])
    if b == 0 or len(rows) == 0:
        z = np.zeros((b, h, w), np.uint8)
        return (z, np.zeros((b, 2), np.int32)) if return_counts else z
    from ._engine import get_engine
    eng = get_engine(device)
    d_rows, d_ptr = eng.upload_hints(rows, ptr)
    _, sel, cnt = eng.wand_select(eng.to_device(imgs), d_rows, d_ptr, *wand.args(), counts=return_counts)
    return (sel.cpu().numpy(), cnt.cpu().numpy()) if return_counts else sel.cpu().numpy()


def wand_select(image: np.ndarray, fg_points, bg_points=(), wand: Optional[Wand] = None, device="cuda") -> np.ndarray:
    """The magic-wand selection of one (H, W, 3) uint8 BGR image (additive; wand_select_batch): fg_points add, bg_points
    subtract.  -> (H, W) uint8, 255 = selected."""
    img = _check_image(image)
    return wand_select_batch(img[None], [(fg_points if fg_points is not None else (), bg_points if bg_points is not None else ())],
                             wand, device=device)[0]


def paint_wand(mask_or_shape, image: np.ndarray, fg_points=(), bg_points=(), wand: Optional[Wand] = None, device="cuda") -> np.ndarray:
    """Magic-wand selections painted into a GrabCut label mask (additive; ggc_wand_select), as
    paint_strokes and paint_polygons paint theirs.  mask_or_shape: an (H, W) uint8 mask of GrabCut labels, or an (H, W)
    shape for a mask that starts all probable background (2).  Every pixel a foreground seed's selection holds becomes
    definite foreground (1), a background seed's definite background (0), background winning where the two overlap;
    every other pixel keeps its label.  -> the painted (H, W) uint8 mask (a copy)."""
    from ._engine import get_engine
    wand = _wand_args(wand)
    img = _check_image(image)
    m = _mask_or_shape(mask_or_shape, "paint_wand")
    if m.shape != img.shape[:2]:
        raise ValueError(f"paint_wand: mask {m.shape} does not match the image {img.shape[:2]}")
    rows, ptr = pack_hints([(fg_points if fg_points is not None else (), bg_points if bg_points is not None else ())])
    if ptr[-1] == 0:
        return m.copy()
    eng = get_engine(device)
    d_rows, d_ptr = eng.upload_hints(rows, ptr)
    md = eng.to_device(m[None])
    eng.wand_select(eng.to_device(img[None]), d_rows, d_ptr, *wand.args(), mask=md, select=False)
    return md[0].cpu().numpy()


@dataclass(frozen=True)
class Outline:
    """One loop of a mask's outline (ggc_mask_outlines, include/ggc.h K1).  vertices: (n, 2) int32
    corners (row, col) of the corner lattice, pixel (y, x) being the square between corners (y, x) and (y+1, x+1), in loop
    order from the loop's smallest corner, the foreground on the right; area: the signed pixel count inside, negative for
    a hole; perimeter: the loop's length in unit steps; outer: the index, in the image's list, of the outer loop of this
    loop's component (an outer loop names itself)."""
    vertices: np.ndarray
    area: int
    perimeter: int
    outer: int

    @property
    def hole(self) -> bool:
        return self.area < 0


def _check_connectivity(connectivity) -> int:
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def mask_outlines_batch(masks, connectivity: int = 8, device="cuda") -> "list[list[Outline]]":
    """The outlines of every mask of a batch (additive; one ggc_mask_outlines call).  masks: (B, H, W), or a sequence of
    equally sized (H, W) masks; any nonzero value is foreground.  -> per image its loops, outer loops and holes, ordered
    by their start (the loop's smallest corner, in raster order)."""
    from ._engine import get_engine
    conn = _check_connectivity(connectivity)
    m = np.asarray(masks)
    if m.ndim != 3:
        raise ValueError(f"mask_outlines_batch: masks must be (B, H, W), got {m.shape}")
    if m.shape[0] == 0:
        return []
    if m.shape[1] < 1 or m.shape[2] < 1:
        raise ValueError(f"mask_outlines_batch: empty masks {m.shape}")
    eng = get_engine(device)
    verts, loop_ptr, info, image_ptr, _ = (t.cpu().numpy() for t in eng.mask_outlines(eng.to_device((m != 0).astype(np.uint8)), conn))
    return [[Outline(verts[loop_ptr[q]:loop_ptr[q + 1]].copy(), int(info[q, 0]), int(info[q, 2]), int(info[q, 1]))
             for q in range(int(image_ptr[b]), int(image_ptr[b + 1]))] for b in range(m.shape[0])]


def mask_outlines(mask, connectivity: int = 8, device="cuda") -> "list[Outline]":
    """The exact vector outlines of one (H, W) mask, any nonzero value foreground (additive; ggc_mask_outlines): crack
    following on the corner lattice.  connectivity 8 joins diagonal foreground pixels into one loop (the components of
    clean_mask), 4 separates them."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError(f"mask_outlines: mask must be (H, W), got {m.shape}")
    return mask_outlines_batch(m[None], connectivity, device)[0]


def outlines_svg_path(outlines) -> str:
    """The loops as one SVG path for fill-rule="evenodd": one `M x y L x y ... Z` sub-path per loop, x = col, y = row."""
    parts = []
    for o in outlines:
        v = np.asarray(o.vertices)
        parts.append("M " + " L ".join(f"{int(c)} {int(r)}" for r, c in v) + " Z")
    return " ".join(parts)


def outlines_to_lassos(outlines) -> "list[np.ndarray]":
    """The outer loops as (row, col) polygons that lasso= / fg_polygons= take (holes are left out)."""
    return [np.asarray(o.vertices, np.int32).copy() for o in outlines if not o.hole]


DIST_FAR = 2 ** 31 - 1                  # GGC_DIST_FAR: the magnitude where no opposite pixel exists, or beyond a cap
MAX_RADIUS2 = 2 * 16384 ** 2            # no two pixels of a 16384 x 16384 image are further apart
MODIFY_OPS = {"grow": 0, "shrink": 1, "border": 2, "open": 3, "close": 4, "trimap": 5}      # ggc_modify_mask's op
_TWO_RADII = (MODIFY_OPS["border"], MODIFY_OPS["trimap"])


def _radius2(radius, radius2, what: str) -> int:
    """A radius as the squared integer radius the device takes: the disk is dy^2 + dx^2 <= floor(radius^2); radius2 gives
    the integer itself (2 is the 8-neighbourhood).  Exactly one of the two."""
    if (radius is None) == (radius2 is None):
        raise ValueError(f"{what}: give either a radius or radius2, got {radius!r} and {radius2!r}")
    if radius2 is not None:
        if isinstance(radius2, (bool, np.bool_)) or not isinstance(radius2, (int, np.integer)) or radius2 < 0:
            raise ValueError(f"{what}: radius2 must be an integer >= 0, got {radius2!r}")
        r2 = int(radius2)
    elif isinstance(radius, (int, np.integer)) and not isinstance(radius, (bool, np.bool_)):
        if radius < 0:
            raise ValueError(f"{what}: radius must be >= 0, got {radius!r}")
        r2 = int(radius) ** 2
    else:
        try:
            r = float(radius)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: radius must be a number, got {radius!r}") from None
        if not np.isfinite(r) or r < 0:
            raise ValueError(f"{what}: radius must be finite and >= 0, got {radius!r}")
        if r * r > 2 * MAX_RADIUS2:
            raise ValueError(f"{what}: radius {radius!r} is beyond any image")
        r2 = int(np.floor(r * r))
    if r2 > MAX_RADIUS2:
        raise ValueError(f"{what}: squared radius {r2} exceeds {MAX_RADIUS2} = 2 * 16384^2")
    return r2


def _radius2_pair(inner, outer, radius2, what: str) -> "tuple[int, int]":
    """The two squared radii of border and trimap: outer None means outer = inner; radius2 an integer (both) or a pair."""
    if radius2 is not None:
        if outer is not None:
            raise ValueError(f"{what}: give either radii or radius2, got outer={outer!r} and radius2={radius2!r}")
        a, b = radius2 if isinstance(radius2, (tuple, list)) and len(radius2) == 2 else (radius2, radius2)
        return _radius2(inner, a, what), _radius2(None, b, what)
    a = _radius2(inner, None, what)
    return a, (a if outer is None else _radius2(outer, None, what))


@dataclass(frozen=True)
class ModifyMask:
    """One step of modify_mask (ggc_modify_mask, include/ggc.h K3).  op: "grow", "shrink", "border", "open",
    "close" or "trimap" (or its number).  radius: an int or float >= 0, the disk being dy^2 + dx^2 <= floor(radius^2), or
    radius2= the squared integer itself.  border and trimap take two radii: radius on the foreground side, outer on the
    background side (None: the same; radius2 may be a pair).  border_background: everything outside the image is
    background, so a shrink also eats from the image's edge."""
    op: "str | int"
    radius: "Optional[float]" = None
    outer: "Optional[float]" = None
    border_background: bool = False
    radius2: "Optional[int | tuple]" = None

    def __post_init__(self):
        self.args()

    def args(self) -> "tuple[int, int, int, bool]":
        """(op, r2_a, r2_b, border_background) as the device takes them; raises ValueError on a bad step."""
        op = MODIFY_OPS.get(self.op.lower()) if isinstance(self.op, str) else (self.op if self.op in MODIFY_OPS.values() else None)
        if op is None:
            raise ValueError(f"ModifyMask: op must be one of {sorted(MODIFY_OPS)}, got {self.op!r}")
        what = f"ModifyMask({self.op!r})"
        if op in _TWO_RADII:
            r2_a, r2_b = _radius2_pair(self.radius, self.outer, self.radius2, what)
        else:
            if self.outer is not None or isinstance(self.radius2, (tuple, list)):
                raise ValueError(f"{what}: only border and trimap take a second radius")
            r2_a, r2_b = _radius2(self.radius, self.radius2, what), 0
        return int(op), r2_a, r2_b, bool(self.border_background)


def _mask_batch(masks, what: str) -> np.ndarray:
    m = np.asarray(masks)
    if m.ndim != 3:
        raise ValueError(f"{what}: masks must be (B, H, W), got {m.shape}")
    if m.shape[0] and (m.shape[1] < 1 or m.shape[2] < 1):
        raise ValueError(f"{what}: empty masks {m.shape}")
    return (m != 0).astype(np.uint8)


def _mask_2d(mask, what: str) -> np.ndarray:
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError(f"{what}: mask must be (H, W), got {m.shape}")
    return m[None]


def mask_distance_batch(masks, signed: bool = True, squared: bool = False, border_background: bool = False,
                        max_distance=None, max_distance2=None, device="cuda") -> np.ndarray:
    """The exact Euclidean distance transform of every mask of a batch (additive; one ggc_mask_distance call).  masks:
    (B, H, W), any nonzero value foreground.  -> (B, H, W) float64: the distance from each background pixel to the nearest
    foreground pixel, and with signed=True minus the distance from each foreground pixel to the nearest background pixel
    (signed=False: its magnitude), inf where there is none; squared=True gives the exact int32 plane instead, DIST_FAR for
    inf.  border_background: everything outside the image is background.  max_distance (or max_distance2, its exact
    square): larger distances are reported as inf and are not searched for."""
    from ._engine import get_engine
    cap2 = None if max_distance is None and max_distance2 is None else _radius2(max_distance, max_distance2, "mask_distance")
    m = _mask_batch(masks, "mask_distance_batch")
    if m.shape[0] == 0:
        return np.zeros(m.shape, np.int32 if squared else np.float64)
    if cap2 == 0:                                                       # every magnitude is at least 1
        d2 = np.where(m != 0, -DIST_FAR, DIST_FAR).astype(np.int32)
    else:
        eng = get_engine(device)
        d2 = eng.mask_distance(eng.to_device(m), border_background, cap2 or 0).cpu().numpy()
    if not signed:
        d2 = np.abs(d2)
    if squared:
        return d2
    mag = np.abs(d2).astype(np.float64)
    dist = np.where(mag == DIST_FAR, np.inf, np.sqrt(mag))
    return np.where(d2 < 0, -dist, dist)


def mask_distance(mask, signed: bool = True, squared: bool = False, border_background: bool = False, max_distance=None,
                  max_distance2=None, device="cuda") -> np.ndarray:
    """The exact Euclidean distance transform of one (H, W) mask: mask_distance_batch of a batch of one."""
    return mask_distance_batch(_mask_2d(mask, "mask_distance"), signed, squared, border_background, max_distance,
                               max_distance2, device)[0]


def modify_mask_batch(masks, *steps: ModifyMask, device="cuda") -> np.ndarray:
    """Apply the steps in order to every mask of a batch, on the device (additive; one ggc_modify_mask call per step, no
    host round trip between them).  masks: (B, H, W), any nonzero value foreground.  -> (B, H, W) uint8 {0, 1}; after a
    trimap step 0 / 128 / 255 (a step after it reads every nonzero value as foreground)."""
    from ._engine import get_engine
    for s in steps:
        if type(s).__name__ != "ModifyMask":                         # by name: the package is importable under two names
            raise ValueError(f"modify_mask: steps must be ModifyMask, got {type(s).__name__}")
    args = [s.args() for s in steps]
    m = _mask_batch(masks, "modify_mask_batch")
    if m.shape[0] == 0 or not args:
        return m
    eng = get_engine(device)
    cur = eng.to_device(m)
    for op, r2_a, r2_b, border in args:
        eng.modify_mask(cur, op, r2_a, r2_b, border, out=cur)           # in place: the row pass never reads the mask
    return cur.cpu().numpy()


def modify_mask(mask, *steps: ModifyMask, device="cuda") -> np.ndarray:
    """Apply the steps in order to one (H, W) mask: modify_mask_batch of a batch of one."""
    return modify_mask_batch(_mask_2d(mask, "modify_mask"), *steps, device=device)[0]


def grow_mask(mask, radius=None, border_background: bool = False, radius2=None, device="cuda") -> np.ndarray:
    """Grow the selection by `radius` pixels: dilation by the exact disk dy^2 + dx^2 <= floor(radius^2) (or radius2)."""
    return modify_mask(mask, ModifyMask("grow", radius, None, border_background, radius2), device=device)


def shrink_mask(mask, radius=None, border_background: bool = False, radius2=None, device="cuda") -> np.ndarray:
    """Shrink the selection by `radius` pixels: erosion by the same disk; border_background also eats from the edge."""
    return modify_mask(mask, ModifyMask("shrink", radius, None, border_background, radius2), device=device)


def open_mask(mask, radius=None, border_background: bool = False, radius2=None, device="cuda") -> np.ndarray:
    """Shrink, then grow: drops specks thinner than the disk."""
    return modify_mask(mask, ModifyMask("open", radius, None, border_background, radius2), device=device)


def close_mask(mask, radius=None, border_background: bool = False, radius2=None, device="cuda") -> np.ndarray:
    """Grow, then shrink: fills pinholes and gaps thinner than the disk."""
    return modify_mask(mask, ModifyMask("close", radius, None, border_background, radius2), device=device)


def border_mask(mask, inner=None, outer=None, border_background: bool = False, radius2=None, device="cuda") -> np.ndarray:
    """The border band of the selection: foreground pixels within `inner` of the background and background pixels within
    `outer` of the foreground (None: outer = inner; radius2 an integer or a pair of squared radii)."""
    return modify_mask(mask, ModifyMask("border", inner, outer, border_background, radius2), device=device)


def mask_to_trimap(mask, inner=None, outer=None, border_background: bool = False, radius2=None, device="cuda") -> np.ndarray:
    """A trimap for trimap_matte from a mask: 255 on the foreground further than `inner` from the background, 0 on the
    background further than `outer` from the foreground, 128 (unknown) on the band between."""
    return modify_mask(mask, ModifyMask("trimap", inner, outer, border_background, radius2), device=device)


@dataclass(frozen=True)
class Scissors:
    """The options of intelligent scissors (ggc_trace_paths, include/ggc.h H4).  margin in 0..256: how
    far, in pixels, a traced segment may leave the bounding box of its two anchors; edge_cap in 1..13770: the gradient
    at which an edge counts as fully strong; smooth in 1..64: the cost per step that does not depend on the image, which
    keeps a path short on flat ground.  The defaults are recorded choices backed by §5.24's study table, not tuned
    results."""
    margin: int = 16
    edge_cap: int = 2048
    smooth: int = 16

    def __post_init__(self):
        for name, lo, hi in (("margin", 0, 256), ("edge_cap", 1, 13770), ("smooth", 1, 64)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"Scissors: {name} must be an integer in [{lo}, {hi}], got {v!r}")


def _scissors_args(options) -> Scissors:
    if options is None:
        return Scissors()
    if not isinstance(options, Scissors):
        raise ValueError(f"scissors options must be a Scissors, got {type(options).__name__}")
    return options


def _vertex_guess(anchors: np.ndarray, n_paths: int) -> int:
    """A guess of the number of traced vertices (Engine.trace_paths' capacity): four times the anchors' Chebyshev spans.
    Too small a guess costs a second call, nothing else."""
    spans = np.abs(np.diff(anchors.astype(np.int64), axis=0)).max(axis=1).sum() if len(anchors) > 1 else 0
    return int(4 * spans + 64 * n_paths)


def _trace_closed(eng, bgr, per_image, options: Scissors) -> "list[list[np.ndarray]]":
    """per_image: one None, anchor list or sequence of anchor lists per image of bgr (B,H,W,3) on the device -> per image
    the traced closed outlines, (n, 2) int32 arrays of (row, col).  An outline of fewer than 3 vertices is a ValueError."""
    b, h, w = int(bgr.size(0)), int(bgr.size(1)), int(bgr.size(2))
    if isinstance(per_image, (str, bytes)) or not hasattr(per_image, "__len__") or len(per_image) != b:
        raise ValueError(f"scissors must have one entry per image of a batch of {b}")
    anchors, path_ptr, closed, image_ptr = pack_paths([scissors_list(s) or None for s in per_image], closed=True)
    if len(closed) == 0:
        return [[] for _ in range(b)]
    if ((anchors < 0) | (anchors >= np.array([h, w]))).any():
        raise ValueError(f"a scissors anchor lies outside the {h}x{w} image")
    verts, vert_ptr = eng.trace_paths(bgr, *eng.upload_paths(anchors, path_ptr, closed, image_ptr), options.margin,
                                      options.edge_cap, options.smooth, capacity=_vertex_guess(anchors, len(closed)))
    verts, vert_ptr = verts.cpu().numpy(), vert_ptr.cpu().numpy()
    out = []
    for i in range(b):
        out.append([verts[vert_ptr[q]:vert_ptr[q + 1]] for q in range(image_ptr[i], image_ptr[i + 1])])
        for k, v in enumerate(out[-1]):
            if len(v) < 3:
                raise ValueError(f"scissors path {k} of image {i} traces {len(v)} vertices: an outline needs at least 3")
    return out


def _merge_lassos(polys: "Optional[tuple]", traced: "list[list[np.ndarray]]") -> "Optional[tuple]":
    """The traced outlines of a batch joined to its packed polygons (or None) as lassos -> packed polygons.  An image's
    traced lassos come before its own polygons; lassos form a union and are painted before every fill, so their place
    among the image's polygons does not matter."""
    if not any(traced):
        return polys
    if polys is None:
        return pack_polygons([((), (), t) if t else None for t in traced])
    verts, pp, pl, ip = polys
    v_out, p_out, l_out, i_out = [], [0], [], [0]
    for i, t in enumerate(traced):
        for v in list(t) + [verts[pp[q]:pp[q + 1]] for q in range(ip[i], ip[i + 1])]:
            v_out.append(np.asarray(v, np.int32).reshape(-1, 2))
            p_out.append(p_out[-1] + len(v))
        l_out += [POLYGON_LASSO] * len(t) + [int(l) for l in pl[ip[i]:ip[i + 1]]]
        i_out.append(len(l_out))
    return (np.ascontiguousarray(np.concatenate(v_out), np.int32), np.asarray(p_out, np.int32), np.asarray(l_out, np.int32),
            np.asarray(i_out, np.int32))


def trace_boundary(image: np.ndarray, anchors, closed: bool = True, scissors: Optional[Scissors] = None,
                   device="cuda") -> np.ndarray:
    """Intelligent scissors on one image (additive; ggc_trace_paths).  image: (H, W, 3) uint8 BGR;
    anchors: (row, col) pairs on the object's outline, in order, inside the image.  Consecutive anchors (and with
    closed=True the last and the first) are joined by the cheapest 8-connected path along image edges that stays within
    scissors.margin pixels of their bounding box.  -> the (n, 2) int32 pixels of the path, (row, col), in order: a
    polygon that lasso= takes as it is."""
    from ._engine import get_engine
    img = _check_image(image)
    opt = _scissors_args(scissors)
    packed = pack_paths([[(anchors, bool(closed))]])
    h, w = img.shape[:2]
    if ((packed[0] < 0) | (packed[0] >= np.array([h, w]))).any():
        raise ValueError(f"trace_boundary: an anchor lies outside the {h}x{w} image")
    eng = get_engine(device)
    verts, _ = eng.trace_paths(eng.to_device(img[None]), *eng.upload_paths(*packed), opt.margin, opt.edge_cap, opt.smooth,
                               capacity=_vertex_guess(packed[0], 1))
    return verts.cpu().numpy()


def lift_labels(mask: np.ndarray, full_shape, band: Optional[int] = None, device="cuda") -> np.ndarray:
    """A working-size mask carried to a larger size as GrabCut labels for a banded cut there (additive; ggc_lift_labels,
    DESIGN.md §5.18).  The mask is interpolated bilinearly (half-pixel centres, as upsample_mask) and thresholded at 0.5;
    the pixels within `band` (Chebyshev) of that lifted mask's edge become probable foreground / background (3 / 2), every
    other pixel definite (1 / 0).

    mask: (H, W) with values in {0, 1}; full_shape: (H1, W1) with H <= H1 <= 32768, W <= W1 <= 32768; band in 0..64, or
    None for one and a half working pixels.  -> (H1, W1) uint8 in {0, 1, 2, 3}."""
    from ._engine import get_engine, check_full_cut_args, default_full_cut_band
    m = _check_cut_mask(mask, "lift_labels")
    full_shape = tuple(int(v) for v in full_shape)
    if len(full_shape) == 2 and band is None and min(full_shape) >= 1:
        band = default_full_cut_band(m.shape, full_shape)
    check_full_cut_args((1, *m.shape), full_shape, band)
    eng = get_engine(device)
    return eng.lift_labels(eng.to_device(m[None]), full_shape, band)[0][0].cpu().numpy()


def _check_cut_mask(mask, what: str) -> np.ndarray:
    m = np.asarray(mask)
    if m.ndim != 2 or m.size == 0:
        raise ValueError(f"{what}: mask must be (H, W), got {m.shape}")
    if m.dtype.kind not in "bui" or not np.isin(m, (0, 1)).all():
        raise ValueError(f"{what}: mask values must be 0 or 1")
    return np.ascontiguousarray(m, np.uint8)


def cut_mask_full(mask: np.ndarray, full_image: np.ndarray, band: Optional[int] = None, n_iter: int = FULL_CUT_ITERS,
                  seed: int = 0, color_space: str = "rgb", min_area_ratio: float = 0.002, keep_largest: bool = False,
                  return_labels: bool = False, device="cuda"):
    """A mask found on a reduced image, cut again on the full-resolution image's own pixels (additive; the banded graph
    cut of Lombaert et al., ICCV 2005).  Four steps on the device: lift_labels(mask, full size, band);
    the colour conversion of GrabCutConfig.color_space; GrabCut from those labels (mode 0, n_iter iterations, cold: the
    colour models are learned on the full image, nothing of the working-size solve is needed); clean_mask.  Outside the
    band the lifted mask stands, so the cost of being wrong is bounded by the band, and a working mask that is off by a
    working pixel is repaired.  A component of the lifted mask thinner than twice the band keeps no definite pixel and
    the cut may delete it: use a smaller band for thin structures.  A mask that lifts to all background or all
    foreground has no band and comes back as it is.

    mask: (H, W) in {0, 1}; full_image: (H1, W1, 3) uint8 BGR, H <= H1 <= 32768, W <= W1 <= 32768, below 2^28 pixels;
    band in 0..64 or None (one and a half working pixels); n_iter in 1..100; color_space rgb | hsv | lab.
    -> (H1, W1) uint8 in {0, 1}; with return_labels, (mask, labels) with the labels GrabCut started from."""
    from ._engine import get_engine, check_full_cut_args, default_full_cut_band
    m = _check_cut_mask(mask, "cut_mask_full")
    full = _check_image(full_image)
    if band is None and min(full.shape[:2]) >= 1:
        band = default_full_cut_band(m.shape, full.shape[:2])
    check_full_cut_args((1, *m.shape), full.shape[:2], band, n_iter, color_space)
    eng = get_engine(device)
    out = eng.cut_mask_full(eng.to_device(m[None]), eng.to_device(full[None]), band, n_iter, int(seed), color_space.lower(),
                            min_area_ratio, keep_largest, want_labels=return_labels)
    if return_labels:
        return out[0][0].cpu().numpy(), out[1][0].cpu().numpy()
    return out[0].cpu().numpy()


def _full_cut_args(full_cut, has_full: bool, matte, shape=None, full_shape=None) -> "Optional[tuple[Optional[int], int]]":
    """(band or None, n_iter) when full_cut is True or a FullCut (checked here, before any stage runs; refused without a
    full image and together with the full-size closed-form solve), else None."""
    if full_cut is None or full_cut is False:
        return None
    if full_cut is True:
        full_cut = FullCut()
    if not isinstance(full_cut, FullCut):
        raise ValueError(f"full_cut must be True, False or a FullCut, got {type(full_cut).__name__}")
    if not has_full:
        raise ValueError("full_cut needs the full image: pass full_image(s) / full_bgr")
    if isinstance(matte, ClosedFormMatte) and matte.full_resolution:
        raise ValueError("full_cut cannot be combined with ClosedFormMatte(full_resolution=True), which defines the full mask "
                         "as its alpha >= 0.5: run with full_cut alone and call closed_form_matte(full_image, "
                         "result.full.binary_mask) for the matte")
    from ._engine import check_full_cut_args
    check_full_cut_args((1, 1, 1) if shape is None else (1, *shape), (1, 1) if full_shape is None else tuple(full_shape),
                        0 if full_cut.band is None else full_cut.band, full_cut.n_iter)
    return (None if full_cut.band is None else int(full_cut.band)), int(full_cut.n_iter)


def nearest_upsample(a: np.ndarray, h1: int, w1: int) -> np.ndarray:
    """(H, W, ...) -> (h1, w1, ...) by the source pixel under each output pixel's centre: index
    min(floor((i + 0.5) * H / h1), H - 1), the centre mapping of upsample_mask."""
    a = np.asarray(a)
    h, w = a.shape[:2]
    ys = np.minimum(((np.arange(h1) + 0.5) * h / h1).astype(np.int64), h - 1)
    xs = np.minimum(((np.arange(w1) + 0.5) * w / w1).astype(np.int64), w - 1)
    return a[ys][:, xs]


def refine_trimap(probs: np.ndarray, segments: np.ndarray, image: np.ndarray, threshold_fg: float = 0.55,
                  threshold_bg: float = 0.55, radius: int = 8, eps: float = 1e-3, device="cuda") -> np.ndarray:
    """Region probabilities -> pixel trimap whose boundaries follow image edges
    (reference pipeline.py:103-146)."""
    from ._engine import get_engine
    eng = get_engine(device)
    p = eng.to_device(np.ascontiguousarray(probs, dtype=np.float32))
    node_ptr = eng.to_device(np.array([0, probs.shape[0]], np.int32))
    seg = eng.to_device(np.ascontiguousarray(segments, dtype=np.int32)[None])
    bgr = eng.to_device(_check_image(image)[None])
    return eng.refine_trimap(p, node_ptr, seg, bgr, threshold_fg, threshold_bg, radius, eps, True)[0].cpu().numpy()


def _seed_from_prior(trimap: np.ndarray, graph, seed_frac: float = 0.1, device="cuda") -> np.ndarray:
    """Guarantee a foreground and a background seed (reference pipeline.py:149-186)."""
    from ._engine import get_engine
    prior = graph.prior_features
    if prior is None or prior.size == 0:
        return trimap
    eng = get_engine(device)
    t = eng.to_device(np.ascontiguousarray(trimap, dtype=np.uint8)[None]).clone()
    p = eng.to_device(np.ascontiguousarray(prior, dtype=np.float32))
    node_ptr = eng.to_device(np.array([0, graph.n_nodes], np.int32))
    seg = eng.to_device(np.ascontiguousarray(graph.segments, dtype=np.int32)[None])
    return eng.seed_from_prior(t, p, node_ptr, seg, seed_frac)[0].cpu().numpy()


def clean_mask(mask: np.ndarray, min_area_ratio: float = 0.002, keep_largest: bool = False, device="cuda") -> np.ndarray:
    """Remove spurious connected components (reference pipeline.py:189-227)."""
    from ._engine import get_engine
    eng = get_engine(device)
    m = eng.to_device(np.ascontiguousarray(mask, dtype=np.uint8)[None])
    return eng.clean_mask(m, min_area_ratio, keep_largest)[0].cpu().numpy()


def eroded_box(H: int, W: int, bbox: tuple[int, int, int, int], ksize: int = 30) -> tuple[int, int, int, int]:
    """(y0, y1, x0, x1) of `cv2.erode(box_mask, np.ones((ksize, ksize)))` for the filled box `bbox` = (x, y, w, h) in an H x W
    image (reference pipeline.py:366-370), in closed form: the kernel's anchor is its centre (ksize // 2), so a pixel survives
    when the ksize pixels from -ksize // 2 to ksize - 1 - ksize // 2 around it are all inside the box; cv2.erode's default
    border counts pixels OUTSIDE the image as set, so a side of the box that lies on the image edge is not eroded."""
    x, y, w, h = bbox
    a, b = ksize // 2, ksize - 1 - ksize // 2
    # the reference fills `inner[y:y+h, x:x+w] = 1` (pipeline.py:368): numpy slice semantics, so a negative start counts from
    # the far edge (and usually selects nothing) and a stop past the frame is cut — the same rows and columns the
    # FG_PROBABLE write of segment_bbox gets
    by0, by1, _ = slice(y, y + h).indices(H)
    bx0, bx1, _ = slice(x, x + w).indices(W)
    if by1 <= by0 or bx1 <= bx0:
        return 0, 0, 0, 0
    y0 = by0 if by0 == 0 else by0 + a
    y1 = by1 if by1 == H else by1 - b
    x0 = bx0 if bx0 == 0 else bx0 + a
    x1 = bx1 if bx1 == W else bx1 - b
    return y0, y1, x0, x1


def _colour_trimap(trimap: np.ndarray) -> np.ndarray:
    """reference pipeline.py:230-236"""
    vis = np.zeros((*trimap.shape, 3), dtype=np.uint8)
    vis[trimap == Label.BG_DEFINITE] = [0, 0, 0]
    vis[trimap == Label.FG_DEFINITE] = [255, 255, 255]
    vis[trimap == Label.BG_PROBABLE] = [60, 20, 20]
    vis[trimap == Label.FG_PROBABLE] = [0, 200, 200]
    return vis


def _host_packed(arg, b: int, name: str, width: int, pack, n_arrays: int, offsets) -> "Optional[tuple]":
    """One hint argument of a batch of b images -> its packed arrays on the host, contiguous int32, the (n, width) rows
    first; None when arg is None.  arg: an already packed tuple of n_arrays arrays or tensors, as `pack` returns it and
    checked here, or one entry per image for `pack`.  offsets(arrays) lists the packing's offset arrays, each as (ptr, its
    name, the number of its ranges, the number of items they share out, the smallest range)."""
    if arg is None:
        return None
    if isinstance(arg, tuple) and len(arg) == n_arrays and all(hasattr(a, "shape") for a in arg) and len(arg[1].shape) == 1:
        arrays = [np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in arg]
        arrays[0] = arrays[0].reshape(-1, width) if arrays[0].size else np.zeros((0, width), np.int32)
        for ptr, ptr_name, n, total, min_step in offsets(arrays):
            if ptr.shape != (n + 1,) or ptr[0] != 0 or (np.diff(ptr) < min_step).any() or ptr[-1] != total:
                raise ValueError(f"packed {name}: {ptr_name} must be a ({n + 1},) array from 0 to {total} in steps of at "
                                 f"least {min_step}")
    else:
        if len(arg) != b:
            raise ValueError(f"{name} has {len(arg)} entries for a batch of {b} images")
        arrays = pack(arg)
    return tuple(np.ascontiguousarray(a, np.int32) for a in arrays)


def _packed_polygons(polygons, b: int) -> "Optional[tuple]":
    """The polygons argument of a batch of b images -> (verts, poly_ptr, poly_label, image_ptr) on the host, or None."""
    return _host_packed(polygons, b, "polygons", 2, pack_polygons, 4,
                        lambda a: [(a[3], "image_ptr", b, len(a[2]), 0), (a[1], "poly_ptr", len(a[2]), len(a[0]), 3)])


def _slice_csr(rows, ptr, lo: int, hi: int):
    """The ranges lo .. hi-1 of a packed list -> (their rows, their offsets from 0)."""
    k0, k1 = int(ptr[lo]), int(ptr[hi])
    return rows[k0:k1], ptr[lo:hi + 1] - k0


@dataclass
class _Hints:
    """The clicks of a batch in ggc_apply_hints' packing, its brush strokes in ggc_apply_strokes' and its polygons in
    ggc_apply_polygons', on the host, and how they are applied."""
    rows: np.ndarray           # (K,3) int32 = row, col, label (1 = foreground)
    ptr: np.ndarray            # (B+1,) int32
    radius: int
    region: bool
    as_prior: bool
    geodesic: "Optional[GeodesicHints]" = None     # set: ggc_geodesic_hints paints the clicks, radius and region do not apply
    segs: Optional[np.ndarray] = None              # (S,5) int32 = r0, c0, r1, c1, label; None: the batch has no stroke
    seg_ptr: Optional[np.ndarray] = None           # (B+1,) int32
    stroke_radius: int = 3
    polys: Optional[tuple] = None                  # (verts, poly_ptr, poly_label, image_ptr) int32; None: the batch has no polygon
    wand_rows: Optional[np.ndarray] = None         # (K,3) int32 wand seeds in ggc_apply_hints' packing; None: the batch has none
    wand_ptr: Optional[np.ndarray] = None          # (B+1,) int32
    wand: "Optional[Wand]" = None                  # the options the seeds are selected with

    @staticmethod
    def of(hints, b: int, radius, region, as_prior, geodesic=None, strokes=None, stroke_radius=3,
           polygons=None, wands=None, wand=None) -> "Optional[_Hints]":
        """hints: one None or (fg_points, bg_points) per image, or an already packed (hints, hint_ptr) pair; strokes: the
        same for brush strokes ((fg_strokes, bg_strokes) per image, or a packed (strokes, stroke_ptr) pair).
        None when no image has a click or a stroke, so that such a call launches exactly what a call without them
        launches; a batch without strokes has segs None and launches exactly what it did before strokes existed.
        polygons: one None or (fg_polygons, bg_polygons, lassos) per image, or a packed 4-tuple (pack_polygons); a batch
        without polygons has polys None and launches exactly what it did before polygons existed.
        wands: one None or (fg_points, bg_points) per image, the seeds of the magic wand, or a packed (seeds, seed_ptr)
        pair; wand: their Wand (None: the defaults).  A batch without wand seeds has wand_rows None and launches exactly
        what it did before the wand existed."""
        geodesic = _geodesic_args(geodesic, region)
        stroked = _host_packed(strokes, b, "strokes", 5, pack_strokes, 2, lambda a: [(a[1], "stroke_ptr", b, len(a[0]), 0)])
        segs, seg_ptr = stroked if stroked is not None and len(stroked[0]) else (None, None)
        polys = _packed_polygons(polygons, b)
        if polys is not None and len(polys[0]) == 0:
            polys = None
        if segs is not None:
            stroke_radius = _check_stroke_radius(stroke_radius)
        wanded = _host_packed(wands, b, "wands", 3, pack_hints, 2, lambda a: [(a[1], "seed_ptr", b, len(a[0]), 0)])
        wand_rows, wand_ptr = wanded if wanded is not None and len(wanded[0]) else (None, None)
        wand = _wand_args(wand) if wand_rows is not None else None
        if hints is None and (segs is not None or polys is not None or wand_rows is not None):   # areas or strokes without clicks: an empty click list
            hints = (np.zeros((0, 3), np.int32), np.zeros(b + 1, np.int32))
        if hints is None:
            return None
        if int(radius) < 0:
            raise ValueError(f"hint_radius must be >= 0, got {radius}")
        rows, ptr = _host_packed(hints, b, "hints", 3, pack_hints, 2, lambda a: [(a[1], "hint_ptr", b, len(a[0]), 0)])
        if len(rows) == 0 and segs is None and polys is None and wand_rows is None:
            return None
        return _Hints(rows, ptr, int(radius), bool(region), bool(as_prior), geodesic, segs, seg_ptr,
                      int(stroke_radius) if segs is not None else 3, polys, wand_rows, wand_ptr, wand)

    def chunk(self, lo: int, hi: int) -> "Optional[_Hints]":
        rows, ptr = _slice_csr(self.rows, self.ptr, lo, hi)
        segs = seg_ptr = polys = wand_rows = wand_ptr = None
        if self.segs is not None:                          # strokes are sliced by stroke_ptr, as clicks by hint_ptr
            segs, seg_ptr = _slice_csr(self.segs, self.seg_ptr, lo, hi)
            if len(segs) == 0:
                segs = seg_ptr = None
        if self.polys is not None:                         # polygons are sliced by image_ptr, their vertices by poly_ptr
            verts, pp, pl, ip = self.polys
            q0, q1 = int(ip[lo]), int(ip[hi])
            if q1 > q0:
                polys = (*_slice_csr(verts, pp, q0, q1), *_slice_csr(pl, ip, lo, hi))
        if self.wand_rows is not None:                     # wand seeds are sliced by seed_ptr, as clicks by hint_ptr
            wand_rows, wand_ptr = _slice_csr(self.wand_rows, self.wand_ptr, lo, hi)
            if len(wand_rows) == 0:
                wand_rows = wand_ptr = None
        if len(rows) == 0 and segs is None and polys is None and wand_rows is None:
            return None
        return _Hints(rows, ptr, self.radius, self.region, self.as_prior, self.geodesic, segs, seg_ptr, self.stroke_radius,
                      polys, wand_rows, wand_ptr, self.wand if wand_rows is not None else None)

    @property
    def has_clicks(self) -> bool:
        """The batch has a click or a stroke: what the click paths (disks, regions, prior columns, geodesic) work on.
        Polygons and wand seeds are areas and feed none of them."""
        return len(self.rows) > 0 or self.segs is not None

    def clicked_images(self, h: int, w: int) -> np.ndarray:
        """(B,) bool: the images with at least one click inside the frame."""
        r, c = self.rows[:, 0], self.rows[:, 1]
        ok = (r >= 0) & (r < h) & (c >= 0) & (c < w)
        img = np.repeat(np.arange(len(self.ptr) - 1), np.diff(self.ptr))
        return np.bincount(img[ok], minlength=len(self.ptr) - 1) > 0


def _full_args(full_bgr, bgr_shape, radius, eps) -> "Optional[tuple[int, float]]":
    """(radius, eps) of the upsample when a full-resolution batch is given (shape and arguments checked here, before any
    stage runs), else None.  full_bgr: the batch or its shape; True when only its presence is known yet."""
    if full_bgr is None:
        return None
    from ._engine import check_matte_args, check_upsample_shapes
    if full_bgr is not True:
        check_upsample_shapes(tuple(bgr_shape), tuple(bgr_shape[:3]), tuple(getattr(full_bgr, "shape", full_bgr)), "full_bgr")
    check_matte_args(radius, eps)
    return int(radius), float(eps)


def _closed_form_args(matte, h: int, w: int, full: bool) -> "Optional[tuple[int, float, int, int, float]]":
    """The closed-form matte's arguments when matte is a ClosedFormMatte (checked here, before any stage runs, with the
    working size h x w, and refused together with full-resolution outputs unless it asks for them itself), else None."""
    if not isinstance(matte, ClosedFormMatte):
        return None
    from ._engine import check_closed_form_args, check_closed_form_shape
    if full and not matte.full_resolution:
        raise ValueError("the closed-form matte is not carried to full resolution: use matte=True with full_image(s), "
                         "or ask for the full-size solve with ClosedFormMatte(full_resolution=True)")
    if matte.full_resolution and not full:
        raise ValueError("ClosedFormMatte(full_resolution=True) needs the full image: pass full_image(s) / full_bgr")
    args = matte.args()
    check_closed_form_args(*args)
    check_closed_form_shape(h, w, args[0])
    _closed_form_full_args(matte)
    return args


def _closed_form_full_args(matte) -> "Optional[tuple[int, int]]":
    """(grow, full_max_iter) when matte is a ClosedFormMatte(full_resolution=True) (checked here), else None."""
    if not (isinstance(matte, ClosedFormMatte) and matte.full_resolution):
        return None
    from ._engine import check_closed_form_args, check_lift_args
    check_closed_form_args(matte.radius, matte.eps, matte.band, matte.full_max_iter, matte.tol)
    check_lift_args((1, 1, 1), None, (1, 1), matte.grow)
    return int(matte.grow), int(matte.full_max_iter)


def _foreground_args(foreground, matte, full: bool) -> "Optional[tuple[float, float, int, float]]":
    """The foreground estimation's arguments when foreground is True or a ForegroundColours (checked here, before any
    stage runs; refused without a matte and together with full-resolution outputs), else None."""
    if foreground is None or foreground is False:
        return None
    if foreground is True:
        foreground = ForegroundColours()
    if not isinstance(foreground, ForegroundColours):
        raise ValueError(f"foreground must be True, False or a ForegroundColours, got {type(foreground).__name__}")
    from ._engine import check_foreground_args
    if not (matte is True or isinstance(matte, ClosedFormMatte)):
        raise ValueError("foreground needs the alpha of a matte: pass matte=True or matte=ClosedFormMatte(...)")
    if full:
        raise ValueError("the foreground colours are not carried to full resolution: drop foreground or full_image(s)")
    args = foreground.args()
    check_foreground_args(*args)
    return args


def _matte_args(matte: bool, radius, eps) -> "Optional[tuple[int, float]]":
    """(radius, eps) when the matte is wanted (checked here, before any stage runs), else None."""
    if not matte:
        return None
    from ._engine import check_matte_args
    check_matte_args(radius, eps)
    return int(radius), float(eps)


# the arguments of segment / segment_batch / segment_batch_device that _OutputPlan.of takes under their own names
_PLAN_OPTIONS = ("compose", "min_area_ratio", "keep_largest", "matte", "matte_radius", "matte_eps", "foreground", "full_cut",
                 "geodesic", "hint_region")


@dataclass(frozen=True)
class _OutputPlan:
    """What one call asked for beyond the cleaned mask, checked: which optional outputs exist and the arguments of the
    entries that fill them.  Built once per call by of(), the one place where an option is refused; _OutputStage runs it."""
    compose: bool                                 # overlay and rgba, at the working size and on the full image
    min_area_ratio: float                         # clean_mask's, also of the full cut
    keep_largest: bool
    mat: "Optional[tuple[int, float]]"            # guided matte: (radius, eps) ...
    cfm: "Optional[tuple[int, float, int, int, float]]"   # ... or the closed-form one: (radius, eps, band, max_iter, tol)
    cff: "Optional[tuple[int, int]]"              # its full-size solve: (grow, full_max_iter)
    fmat: "Optional[tuple[int, float]]"           # the upsample's (radius, eps); set exactly when there is a full image
    fga: "Optional[tuple[float, float, int, float]]"      # foreground colours: (eps_r, omega, max_iter, tol)
    fcut: "Optional[tuple[Optional[int], int]]"   # full cut: (band or None for the default, n_iter), on seed and color_space
    seed: int
    color_space: str

    @classmethod
    def of(cls, pipe, shape, full, compose: bool = True, min_area_ratio: float = 0.002, keep_largest: bool = False,
           matte=False, matte_radius=MATTE_RADIUS, matte_eps=MATTE_EPS, foreground=False, full_cut=False, geodesic=False,
           hint_region: bool = False) -> "_OutputPlan":
        """shape: (B,H,W,3) of the working batch; full: the (B,H1,W1,3) shape of the full images, None without them, or
        True when they are given but not read yet (segment_batch refuses options before it looks at its list; the shape
        checks are then left to the call that knows it).  A call that is wrong in several ways is refused for the first
        of: hints, closed-form matte, guided matte, full image, foreground, full-size closed form, full cut.  pipe, whose
        GrabCutConfig gives the seed and the colour space, is not touched before all of them had their chance."""
        has_full, sized = full is not None, full is not None and full is not True
        _geodesic_args(geodesic, hint_region)
        cfm = _closed_form_args(matte, shape[1], shape[2], has_full)
        mat = None if cfm else _matte_args(matte, matte_radius, matte_eps)
        fmat = _full_args(full, shape, matte_radius, matte_eps)
        fga = _foreground_args(foreground, matte, has_full)
        cff = _closed_form_full_args(matte) if cfm else None
        fcut = _full_cut_args(full_cut, has_full, matte, shape[1:3] if sized else None, full[1:3] if sized else None)
        cs = pipe.gc_config.color_space.lower()
        if cs not in ("rgb", "hsv", "lab"):
            raise ValueError(f"unknown color_space '{cs}': rgb | hsv | lab")
        return cls(bool(compose), min_area_ratio, keep_largest, mat, cfm, cff, fmat, fga, fcut, pipe.gc_config.seed, cs)


class _OutputStage:
    """Everything after GrabCut for one batch under one _OutputPlan.  It owns the output buffers; run() issues the work of
    images lo:hi on whatever engine and stream the caller is on (a GrabCut lane, a chunk's lane, or the caller's own), so
    the schedules differ only in who calls it and when.  final_mask: (B,H,W) uint8 masks that are final already
    (segment_bbox: GrabCut's own, with its own overlay); they stand in for the cleaned masks, from_mask() is the entry,
    and there is no working-size overlay."""

    def __init__(self, eng, plan: _OutputPlan, bgr, full_bgr=None, final_mask=None):
        import torch
        self.plan, self.bgr, self.full_bgr = plan, bgr, full_bgr

        def u8(shape, *channels):
            return eng.empty(*shape, *channels, dtype=torch.uint8)

        def buffers(shape, compose, matte) -> dict:
            out = {}
            if compose:
                out["overlay"], out["rgba"] = u8(shape, 3), u8(shape, 4)
            if matte:
                out["alpha"], out["rgba_soft"] = eng.empty(*shape), u8(shape, 4)
            return out

        shape = tuple(bgr.shape[:3])
        self.cleaned = u8(shape) if final_mask is None else final_mask
        # the optional entries of segment_batch_device's dict, in its order
        self.out = buffers(shape, plan.compose and final_mask is None, plan.mat or plan.cfm)
        if plan.fga:
            self.out["foreground"], self.out["rgba_clean"] = u8(shape, 3), u8(shape, 4)
        if full_bgr is not None:
            full_shape = tuple(full_bgr.shape[:3])
            self.out["full"] = {"binary_mask": u8(full_shape), **buffers(full_shape, plan.compose, plan.mat or plan.cff)}

    def run(self, leng, lo: int, hi: int, binary_part) -> None:
        """Images lo:hi from GrabCut's binary masks binary_part: ggc_clean_mask, ggc_compose_outputs, then from_mask."""
        p, o = self.plan, self.out
        leng.clean_mask(binary_part, p.min_area_ratio, p.keep_largest, out=self.cleaned[lo:hi])
        if p.compose:
            leng.compose(self.bgr[lo:hi], self.cleaned[lo:hi], out=(o["overlay"][lo:hi], o["rgba"][lo:hi]))
        self.from_mask(leng, lo, hi)

    def from_mask(self, leng, lo: int, hi: int) -> None:
        """What follows the final masks of images lo:hi.  alpha and rgba_soft: the guided matte (mat) or the closed-form one
        (cfm); the foreground colours under that alpha (fga).  With a full image, its outputs: ggc_upsample_matte, then
        ggc_compose_outputs on the full image and the upsampled mask.  With cff (ClosedFormMatte(full_resolution=True))
        the alpha comes from the full-size closed-form solve instead, warm from the working-size alpha on its lifted
        band, and the mask is that alpha >= 0.5 (closed_form_matte_full).  With fcut (full_cut) the mask is
        cut_mask_full of the final mask, image b on seed + b; the alpha, if wanted, stays the guided upsample's."""
        import torch
        p, o = self.plan, self.out
        img, cleaned = self.bgr[lo:hi], self.cleaned[lo:hi]
        if p.mat:
            leng.alpha_matte(img, cleaned, *p.mat, want_rgba=True, out=(o["alpha"][lo:hi], o["rgba_soft"][lo:hi]))
        elif p.cfm:
            leng.closed_form_matte(img, cleaned, *p.cfm, out=(o["alpha"][lo:hi], o["rgba_soft"][lo:hi]))
        if p.fga:
            leng.estimate_foreground(img, o["alpha"][lo:hi], *p.fga, out=(o["foreground"][lo:hi], o["rgba_clean"][lo:hi]))
        if "full" not in o:
            return
        full, big = o["full"], self.full_bgr[lo:hi]
        mask = full["binary_mask"][lo:hi]
        alpha, soft = (full[k][lo:hi] if k in full else None for k in ("alpha", "rgba_soft"))
        if p.fcut:
            from ._engine import default_full_cut_band
            band, n_iter = p.fcut
            if band is None:
                band = default_full_cut_band(cleaned.shape[1:], big.shape[1:3])
            if alpha is not None:
                leng.upsample_matte(img, cleaned, big, *p.fmat, out=(alpha, None, soft))
            leng.cut_mask_full(cleaned, big, band, n_iter, p.seed + lo, p.color_space, p.min_area_ratio, p.keep_largest,
                               out=mask, max_pixels=FULL_CUT_PIXELS)
        elif p.cff:
            radius, eps, band, _, tol = p.cfm
            leng.closed_form_full(img, leng.closed_form_band(cleaned, band), o["alpha"][lo:hi], big, radius, eps, *p.cff, tol,
                                  out=(alpha, soft))
            mask.copy_(torch.ge(alpha, 0.5))
        else:
            leng.upsample_matte(img, cleaned, big, *p.fmat, out=(alpha, mask, soft))
        if p.compose:
            leng.compose(big, mask, out=(full["overlay"][lo:hi], full["rgba"][lo:hi]))

    def result(self, trimap, segments, graphs, probs, gc_mask, state: "Optional[dict]" = None) -> dict:
        """segment_batch_device's dict: the front stages' tensors, GrabCut's state when it was asked for, this stage's outputs."""
        return {"binary_mask": self.cleaned, "trimap": trimap, "segments": segments, "graphs": graphs, "probs": probs,
                "gc_mask": gc_mask, **(state or {}), **self.out}


_REFERENCE_FIELDS = ("binary_mask", "trimap", "segments", "overlay", "rgba")     # of SegmentationResult, as keys of the dict
_ADDITIVE_FIELDS = ("alpha", "rgba_soft", "foreground", "rgba_clean")


def _optional_results(out: dict, i: int) -> dict:
    """The additive fields of image i's SegmentationResult that the device dict `out` holds."""
    res = {k: out[k][i].cpu().numpy() for k in _ADDITIVE_FIELDS if k in out}
    if "full" in out:
        host = {k: v[i].cpu().numpy() for k, v in out["full"].items()}
        res["full"] = FullResolution(binary_mask=host["binary_mask"], overlay=host.get("overlay"), rgba=host.get("rgba"),
                                     alpha=host.get("alpha"), rgba_soft=host.get("rgba_soft"))
    return res


def _result(out: dict, i: int, image: np.ndarray, timing: dict) -> SegmentationResult:
    """Image i of segment_batch_device's dict as a SegmentationResult on the host."""
    return SegmentationResult(image=image, timing=timing, **_optional_results(out, i),
                              **{k: out[k][i].cpu().numpy() if k in out else None
                                 for k in _REFERENCE_FIELDS})


class GCNGrabCutPipeline:
    """
    Full GCN-GrabCut segmentation pipeline on the MI355X (reference pipeline.py:239-380).

    model     : trimap predictor (ResGCNNet)
    sp_config : SuperpixelGraphConfig (default 300 segments)
    gc_config : GrabCutConfig (default 5 iterations)
    device    : "cuda" / "cuda:<i>"
    """

    def __init__(self, model, sp_config: Optional[SuperpixelGraphConfig] = None,
                 gc_config: Optional[GrabCutConfig] = None, device: str = "cuda", grabcut_lanes: int = 4, engine=None,
                 chunks: int = 1, chunk_ratio: float = 0.8):
        from ._engine import get_engine
        self._eng = engine if engine is not None else get_engine(device)
        self.grabcut_lanes = int(grabcut_lanes)   # additive: concurrent sub-batches of the GrabCut stage (batched calls only)
        self.chunks = int(chunks)                 # additive: chunks of the software pipeline of segment_batch_device (1 = off, the default: measured no faster)
        self.chunk_ratio = float(chunk_ratio)
        self.model = model.to(self._eng.device)
        self.device = device
        self.sp_config = sp_config or SuperpixelGraphConfig()
        self.gc_config = gc_config or GrabCutConfig()
        self._replicas = None

    def replica(self, grabcut_lanes: int = 1) -> "GCNGrabCutPipeline":
        """Additive: a pipeline over the same model with a private library context (own scratch arena), so that it can
        run CONCURRENTLY with this one from another host thread on another HIP stream — batch k+1's SLIC / graph / GCN
        stages then run under batch k's GrabCut, whose max-flow leaves most of the GPU idle."""
        from ._engine import Engine
        return GCNGrabCutPipeline(self.model, self.sp_config, self.gc_config, self.device, grabcut_lanes,
                                  engine=Engine(self._eng.index, private_context=True))

    def segment_batches_overlapped(self, batches: Sequence, n_pipelines: int = 3, **kwargs) -> list[dict]:
        """Additive: segment_batch_device() over several (B,H,W,3) uint8 device tensors with up to n_pipelines of them
        in flight at once (this pipeline + replicas, one host thread and HIP stream each, one GrabCut lane each).
        Results are those of one-at-a-time calls, in input order; on one MI355X three pipelines move ~25 % more
        images per second than one pipeline with four GrabCut lanes."""
        import threading
        import torch
        batches = list(batches)
        n = max(1, min(int(n_pipelines), len(batches)))
        if n == 1:
            return [self.segment_batch_device(b, **kwargs) for b in batches]
        if getattr(self, "_replicas", None) is None or len(self._replicas) < n - 1:
            self._replicas = [self.replica(grabcut_lanes=1) for _ in range(n - 1)]
            self._streams = [torch.cuda.Stream(self._eng.device) for _ in range(n)]
        pipes = [self] + self._replicas[:n - 1]
        caller = torch.cuda.current_stream(self._eng.device)
        out: list = [None] * len(batches)
        errors: list = []

        def worker(i):
            try:
                torch.cuda.set_device(self._eng.device)
                self._streams[i].wait_stream(caller)               # the batches were produced on the caller's stream
                with torch.cuda.stream(self._streams[i]):
                    for k in range(i, len(batches), n):
                        out[k] = pipes[i].segment_batch_device(batches[k], grabcut_lanes=1, **kwargs)
                self._streams[i].synchronize()
            except Exception as exc:                               # re-raised in the caller's thread
                errors.append(exc)

        threads = [threading.Thread(target=worker, args=(i,), name=f"ggc-pipe{i}") for i in range(n)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise errors[0]
        for o in out:                                              # the results were allocated on the side streams
            for v in o.values():
                for t_ in (vars(v).values() if hasattr(v, "__dict__") and not torch.is_tensor(v) else (v,)):
                    if torch.is_tensor(t_) and t_.is_cuda:
                        t_.record_stream(caller)
        return out

    # ------------------------------------------------------------ batched, device resident
    def _front(self, eng, bgr, threshold_fg, threshold_bg, edge_aware, filter_radius, tick=None, timing=None, hints=None):
        """Stages 1-3 on the current stream: colour prep, SLIC, graph, network, trimap, seeding, then the user's clicks
        (hints: a _Hints or None).  Polygons (ggc_apply_polygons), then wand selections (ggc_wand_select), are painted
        after the seeding and before strokes and clicks, so a stroke or click inside an excluded area still wins, being
        the more specific edit; they are areas, not clicks, and do not feed hint_region, hints_as_prior or the geodesic
        sources.  -> (seg, graphs, probs, trimap)"""
        cfg = self.sp_config
        t = tick() if tick else 0.0
        lab, hsv, gray, grad = eng.preprocess(bgr)
        seg, n_nodes = eng.slic(lab, cfg.n_segments, cfg.compactness, cfg.sigma) if cfg.use_lab else \
            eng.slic_rgb(bgr, cfg.n_segments, cfg.compactness, cfg.sigma)          # reference graph_builder.py:177-179
        graphs = eng.build_graphs(seg, n_nodes, lab, hsv, grad, cfg.connectivity, cfg.n_nonlocal)
        if timing is not None:
            timing["graph_build"] = tick() - t
            timing["data_prep"] = 0.0          # the graph is already in HBM: nothing to copy
        t = tick() if tick else 0.0
        if self.model.training:
            self.model.eval()
        prior = graphs.x[:, 16:19]
        polys = None if hints is None else hints.polys
        wands = None if hints is None or hints.wand_rows is None else (hints.wand_rows, hints.wand_ptr, hints.wand)
        if hints is not None and not hints.has_clicks:     # areas only: the click paths launch nothing
            hints = None
        dev = None                             # the device copies _paint_hints works on
        if hints is not None:
            hint_rows, hint_ptr = eng.upload_hints(hints.rows, hints.ptr)
            all_rows, all_ptr, clicked = hint_rows, hint_ptr, None     # what the superpixels, the prior and the geodesic see
            segs = seg_ptr = None
            if hints.segs is not None:
                segs, seg_ptr = eng.upload_strokes(hints.segs, hints.seg_ptr)
                if hints.as_prior or hints.region or hints.geodesic is not None:
                    all_rows, all_ptr, clicked = self._with_stroke_pixels(eng, hints, hint_rows, seg.shape, segs, seg_ptr)
            if hints.as_prior:
                prior = self._hints_as_prior(eng, hints, all_rows, all_ptr, seg, graphs, bgr, clicked)
            dev = (hint_rows, hint_ptr, all_rows, all_ptr, segs, seg_ptr)
        probs = eng.predict_probs(self.model, graphs)
        trimap = eng.refine_trimap(probs, graphs.node_ptr, seg, bgr, threshold_fg, threshold_bg, filter_radius,
                                   1e-3, edge_aware)
        if timing is not None:
            timing["gcn_inference"] = tick() - t
        trimap = eng.seed_from_prior(trimap, prior, graphs.node_ptr, seg, 0.1)
        self._paint_hints(eng, trimap, polys, hints, dev, bgr, seg, graphs.node_ptr, wands)
        return seg, graphs, probs, trimap

    @staticmethod
    def _paint_hints(eng, trimap, polys, hints, dev, bgr, seg, node_ptr, wands=None):
        """The user's edits as hard constraints on the seeded trimap, in place: polygons, then wand selections, then the
        strokes and clicks.  Areas come first and the more precise tools go on top."""
        if polys is not None:                  # areas first: lassos, then fills; strokes and clicks are painted over them
            eng.apply_polygons(trimap, *eng.upload_polygons(*polys))
        if wands is not None:                  # (seeds, seed_ptr, Wand) on the host; the guide is the caller's BGR batch, never gc_image
            eng.wand_select(bgr, *eng.upload_hints(wands[0], wands[1]), *wands[2].args(), mask=trimap, select=False)
        if hints is None:
            return
        hint_rows, hint_ptr, all_rows, all_ptr, segs, seg_ptr = dev
        if hints.geodesic is not None:         # the guide is the caller's BGR batch, never gc_image
            eng.geodesic_hints(bgr, all_rows, all_ptr, hints.geodesic.radius, hints.geodesic.gamma, mask=trimap)
        elif hints.segs is None:               # hard constraints: over the network's trimap and the seeding alike
            eng.apply_hints(trimap, hint_rows, hint_ptr, hints.radius, hints.region, seg, node_ptr)
        else:                                  # strokes: the superpixels under centre lines and clicks, the brush, the disks
            if hints.region:
                eng.apply_hints(trimap, all_rows, all_ptr, 0, True, seg, node_ptr)
            eng.apply_strokes(trimap, segs, seg_ptr, hints.stroke_radius)
            if len(hints.rows):
                eng.apply_hints(trimap, hint_rows, hint_ptr, hints.radius, False)

    @staticmethod
    def _with_stroke_pixels(eng, hints, hint_rows, shape, segs, seg_ptr):
        """The merged click list of a stroked batch on the device: per image its strokes' centre-line pixels
        (ggc_stroke_pixels), then its clicks.  -> (rows, ptr, (B,) bool: the images with a stroke pixel or a click inside
        the frame)."""
        import torch
        pix, pix_ptr = eng.stroke_pixels(tuple(shape), segs, seg_ptr)
        pp, cp = pix_ptr.cpu().numpy().astype(np.int64), hints.ptr.astype(np.int64)
        clicked = (np.diff(pp) > 0) | hints.clicked_images(shape[1], shape[2])
        if cp[-1] == 0:
            return pix, pix_ptr, clicked
        n_pix = int(pp[-1])
        src = np.concatenate([np.concatenate([np.arange(pp[b], pp[b + 1]), n_pix + np.arange(cp[b], cp[b + 1])])
                              for b in range(len(pp) - 1)])
        rows = torch.cat([pix, hint_rows])[eng.to_device(src)].contiguous()
        return rows, eng.to_device((pp + cp).astype(np.int32)), clicked

    @staticmethod
    def _hints_as_prior(eng, hints, hint_rows, hint_ptr, seg, graphs, bgr=None, clicked=None):
        """The reference's use of encode_user_hints: the prior columns x[:, 16:19] of every image with a click inside the
        frame become its click table; the other images keep the automatic prior.  Returns a copy of the automatic prior,
        which seed_from_prior still reads.  Geodesic hints: the table is encode_geodesic_hints', computed on the host
        in float64 from the per-superpixel distances of ggc_geodesic_hints."""
        import torch
        auto = graphs.x[:, 16:19].clone()
        if hints.geodesic is not None:
            from .graph_builder import geodesic_prior_columns
            g = hints.geodesic
            nd = eng.empty(graphs.x.size(0), 2, dtype=torch.int32)
            eng.geodesic_hints(bgr, hint_rows, hint_ptr, g.radius, g.gamma, segments=seg, node_ptr=graphs.node_ptr, node_dist=nd)
            table = eng.to_device(geodesic_prior_columns(nd.cpu().numpy(), g.radius, g.sigma))
        else:
            table = eng.empty(graphs.x.size(0), 3)
            eng.apply_hints(None, hint_rows, hint_ptr, segments=seg, node_ptr=graphs.node_ptr, node_hints=table, shape=seg.shape)
        if clicked is None:                    # (given with strokes: their centre-line pixels count as clicks)
            clicked = hints.clicked_images(seg.size(1), seg.size(2))
        nptr = graphs.node_ptr_host
        b = 0
        while b < len(clicked):                # one copy per run of consecutive clicked images
            if not clicked[b]:
                b += 1
                continue
            e = b
            while e < len(clicked) and clicked[e]:
                e += 1
            n0, n1 = int(nptr[b]), int(nptr[e])
            graphs.x[n0:n1, 16:19] = table[n0:n1]
            b = e
        return auto

    @staticmethod
    def chunk_plan(b: int, n_chunks: int, ratio: float = 0.8) -> list[tuple[int, int]]:
        """Contiguous chunks of a batch for the software pipeline, each `ratio` times the size of the one before it: the
        GrabCut of a chunk starts when its trimaps exist, so later chunks start later and get fewer images to end together."""
        n_chunks = max(1, min(int(n_chunks), b))
        w = [ratio ** k for k in range(n_chunks)]
        cuts, acc = [0], 0.0
        for k in range(n_chunks - 1):
            acc += w[k]
            cuts.append(min(b - (n_chunks - 1 - k), max(cuts[-1] + 1, int(round(b * acc / sum(w))))))
        cuts.append(b)
        return [(cuts[k], cuts[k + 1]) for k in range(n_chunks)]

    def segment_batch_device(self, bgr, threshold_fg: float = 0.55, threshold_bg: float = 0.55,
                             refine_iters: int = 0, min_area_ratio: float = 0.002, keep_largest: bool = False,
                             edge_aware: bool = True, filter_radius: int = 8, compose: bool = True,
                             timing: Optional[dict] = None, grabcut_lanes: Optional[int] = None,
                             chunks: Optional[int] = None, hints=None, hint_radius: int = 5, hint_region: bool = False,
                             hints_as_prior: bool = False, return_state: bool = False, matte: bool = False,
                             matte_radius: int = MATTE_RADIUS, matte_eps: float = MATTE_EPS, full_bgr=None,
                             foreground=False, full_cut=False, geodesic=False, strokes=None, stroke_radius: int = 3,
                             polygons=None, scissors=None, scissors_options=None, wands=None, wand=None) -> dict:
        """bgr: (B,H,W,3) uint8 tensor on the pipeline's device.  Returns device tensors.

        matte=True (additive) also returns "alpha" (B,H,W) float32, the soft matte of the cleaned mask (alpha_matte with
        matte_radius / matte_eps), and "rgba_soft" (B,H,W,4) uint8, the cut-out with that alpha.  Every other output is
        the same as without it.  matte=ClosedFormMatte(...) fills the same two outputs with closed_form_matte of the
        cleaned mask instead (matte_radius / matte_eps do not apply); it cannot be combined with full_bgr unless it says
        full_resolution=True, and then "full" holds "alpha" and "rgba_soft" of closed_form_matte_full and "binary_mask"
        = that alpha >= 0.5 (with "overlay" / "rgba" composed from it); every working-size output stays the same.

        foreground=True or ForegroundColours(...) (additive, needs a matte) also returns "foreground" (B,H,W,3) uint8,
        the estimated foreground colours under that matte's alpha (estimate_foreground), and "rgba_clean" (B,H,W,4)
        uint8, the cut-out with those colours and the byte round(255 alpha) of that alpha.  Every other output is the
        same as without it; it cannot be combined with full_bgr.

        full_bgr (additive): a (B,H1,W1,3) uint8 tensor on the device, the same images at a resolution of at least the
        working one.  The result then also has "full", a dict of device tensors at (H1, W1): "binary_mask", the cleaned
        mask carried to the full image by upsample_mask (with matte_radius / matte_eps), and "overlay" / "rgba" composed
        from it (compose=True), plus "alpha" and "rgba_soft" with matte=True.  Every other output is the same as without
        it.  full_cut=True or FullCut(...) (additive, needs full_bgr) makes that "binary_mask" cut_mask_full of the cleaned
        mask instead, a banded graph cut on the full image (GrabCutConfig.color_space, this call's min_area_ratio and
        keep_largest, image b on GrabCutConfig.seed + b), with "overlay" / "rgba" composed from it; "alpha" and
        "rgba_soft" stay the guided upsample's.  It cannot be combined with ClosedFormMatte(full_resolution=True).

        return_state=True (additive) also returns what a GC_EVAL edit loop continues from: "gc_binary" (B,H,W) uint8,
        GrabCut's own binary mask before clean_mask; "bgd" / "fgd" (B,65) float64, the colour models; "gc_image"
        (B,H,W,3) uint8, the image in GrabCutConfig.color_space (bgr itself for "rgb").  "gc_mask" is returned either way.

        User clicks (additive): hints is None, a list with one None or (fg_points, bg_points) per image ((row, col) pairs,
        as encode_user_hints takes them), or a packed (hints, hint_ptr) pair (graph_builder.pack_hints).  They are hard
        constraints on the trimap GrabCut is given (ggc_apply_hints, after the seeding): every pixel within hint_radius of
        a click becomes definite foreground / background, the later click winning where disks overlap; hint_region=True
        first does the same for every superpixel whose clicks all carry one label.  hints_as_prior=True also replaces the
        network's prior columns x[:, 16:19] of each image with a click in the frame by encode_user_hints.  clean_mask
        still runs after GrabCut, so a foreground click on a component smaller than min_area_ratio can be removed.
        geodesic=True or GeodesicHints(...) (additive) paints the clicks by ggc_geodesic_hints instead: a pixel becomes
        definite where its geodesic distance on bgr to the nearest click of a label is within the cap and below the
        distance to every click of the other label.  hint_radius is ignored in geodesic mode,
        hint_region=True is a ValueError, and hints_as_prior=True then writes encode_geodesic_hints' soft columns (an
        encoding no shipped network was trained on).  Without clicks the option launches nothing.

        Brush strokes (additive): strokes is None, a list with one None or (fg_strokes, bg_strokes) per
        image (each a sequence of strokes, a stroke a sequence of (row, col) vertices), or a packed (strokes, stroke_ptr)
        pair (graph_builder.pack_strokes).  Every pixel within stroke_radius of a stroke becomes definite foreground /
        background (ggc_apply_strokes; radius 0: the centre line; the part of a stroke inside the image is painted), the
        later segment winning, then the clicks' disks are painted over the strokes.  With hint_region / hints_as_prior a
        stroke's centre-line pixels (ggc_stroke_pixels) count as clicks before the image's own: a stroke claims every
        superpixel its centre line crosses.  In geodesic mode the centre line is the source set and stroke_radius is
        ignored, as hint_radius is.  A batch without strokes launches exactly what it did before, and an image without
        strokes in a stroked batch gets the outputs it gets without them, bit for bit.

        Lassos and filled polygons (additive): polygons is None, a list with one None or (fg_polygons,
        bg_polygons, lassos) per image (each a sequence of polygons, a polygon a sequence of n >= 3 (row, col) vertices,
        closed implicitly), or a packed (verts, poly_ptr, poly_label, image_ptr) tuple (graph_builder.pack_polygons).  On
        the trimap GrabCut starts from, every pixel outside all of an image's lassos becomes definite background, then
        every pixel a fill covers definite foreground / background (ggc_apply_polygons: even-odd rule, boundary included,
        the later fill winning, background fills after foreground ones); strokes and clicks are painted afterwards, so
        one inside an excluded area still wins.  Polygons are areas, not clicks: they do not feed hint_region,
        hints_as_prior or the geodesic sources.  A batch without polygons launches exactly what it did before, and an
        image without polygons in a batch that has some gets the outputs it gets without them, bit for bit.

        Intelligent scissors (additive): scissors is None or a list with, per image, None, one anchor
        list ((row, col) pairs on the object's outline, in order, inside the image) or a sequence of anchor lists;
        scissors_options is a Scissors (None: its defaults).  Each anchor list is traced as a closed path on bgr, the
        working-size BGR image and never GrabCutConfig's colour-space image (ggc_trace_paths), and the traced outlines
        join the image's lassos: the union rule above applies and they are painted where lassos are painted, so the
        result equals that of passing trace_boundary's polygons as lassos.  An outline of fewer than 3 vertices is a
        ValueError.  A batch without scissors launches exactly what it did before.

        Magic wand (additive): wands is None, a list with one None or (fg_points, bg_points) per image
        ((row, col) seeds), or a packed (seeds, seed_ptr) pair (graph_builder.pack_hints); wand is a Wand (None: its
        defaults).  On the trimap GrabCut starts from, every pixel that a seed selects on bgr, the working-size BGR image
        and never GrabCutConfig's colour-space image (ggc_wand_select), becomes definite foreground / background, an
        image's later seed winning, background seeds after foreground ones.  Selections are painted after the polygons
        and before strokes and clicks.  Wand seeds are areas, not clicks: they do not feed hint_region, hints_as_prior or
        the geodesic sources.  A batch without wand seeds launches exactly what it did before, and an image without them
        in a batch that has some gets the outputs it gets without them, bit for bit.

        Large batches run as a software pipeline (additive, same results): the batch is cut into `chunks` contiguous
        chunks; the front stages of chunk k+1 run on the caller's stream while the GrabCut / clean-up of chunk k runs on a
        lane of its own (private context, stream and host thread).  Images are independent and image b keeps seed + b, so
        every output equals the one-chunk run bit for bit."""
        import torch
        eng = self._eng
        b = bgr.size(0)
        want = self.grabcut_lanes if grabcut_lanes is None else int(grabcut_lanes)   # (an argument, so that concurrent callers do not mutate the pipeline)
        n_chunks = self.chunks if chunks is None else int(chunks)
        if scissors is not None:                   # traced once for the whole batch; from here on they are lassos
            polygons = _merge_lassos(_packed_polygons(polygons, b),
                                     _trace_closed(eng, bgr, scissors, _scissors_args(scissors_options)))
        hints = _Hints.of(hints, b, hint_radius, hint_region, hints_as_prior, geodesic, strokes, stroke_radius, polygons,
                          wands, wand)
        plan = _OutputPlan.of(self, bgr.shape, None if full_bgr is None else full_bgr.shape, compose=compose,
                              min_area_ratio=min_area_ratio, keep_largest=keep_largest, matte=matte, matte_radius=matte_radius,
                              matte_eps=matte_eps, foreground=foreground, full_cut=full_cut)
        cs = plan.color_space
        if n_chunks <= 0:                          # 0: one chunk per GrabCut lane once every chunk gets a lane's worth of images
            n_chunks = max(want, 1) if b >= 16 * max(want, 1) else 1
        if n_chunks > 1 and b >= 2 * n_chunks:
            return self._segment_pipelined(bgr, full_bgr, self.chunk_plan(b, n_chunks, self.chunk_ratio), plan, threshold_fg,
                                           threshold_bg, refine_iters, edge_aware, filter_radius, timing, hints, return_state)

        def tick():
            if timing is not None:
                torch.cuda.synchronize(eng.device)
            return time.perf_counter()

        seg, graphs, probs, trimap = self._front(eng, bgr, threshold_fg, threshold_bg, edge_aware, filter_radius, tick, timing,
                                                 hints)

        t = tick()
        mask = trimap.clone()
        lanes = self._lane_count(b, want)
        gc_img = bgr if cs == "rgb" else eng.convert_color8(bgr, cs)      # reference grabcut.py:73-79
        # the output stage is per image: without stage timing each GrabCut lane runs it for its own sub-batch as soon as
        # it is cut (on its stream, under the other lanes' tails); with timing it stays a stage of its own
        stage = _OutputStage(eng, plan, bgr, full_bgr)
        fused_post = timing is None
        binary, mask, bgd, fgd = eng.grabcut_lanes(gc_img, mask, self.gc_config.n_iter, 0, self.gc_config.seed, lanes,
                                                   post=stage.run if (fused_post and refine_iters <= 0) else None)
        if refine_iters > 0:
            binary, mask, bgd, fgd = eng.grabcut_lanes(gc_img, mask, refine_iters, 2, self.gc_config.seed, lanes, bgd, fgd,
                                                       post=stage.run if fused_post else None)
        if timing is not None:
            timing["grabcut"] = tick() - t

        t = tick()
        if not fused_post:
            stage.run(eng, 0, b, binary)
        out = stage.result(trimap, seg, graphs, probs, mask,
                           dict(gc_binary=binary, bgd=bgd, fgd=fgd, gc_image=gc_img) if return_state else None)
        if timing is not None:
            timing["postprocess"] = tick() - t
        return out

    def _lane_count(self, b: int, want: Optional[int] = None) -> int:
        """The GrabCut lanes a batch of b images runs on: the wanted number once every lane gets eight images, else one."""
        want = max(self.grabcut_lanes if want is None else want, 1)
        return want if b >= 8 * want else 1

    def _segment_pipelined(self, bgr, full_bgr, chunks, plan, threshold_fg, threshold_bg, refine_iters, edge_aware,
                           filter_radius, timing, hints=None, return_state=False) -> dict:
        """The software pipeline behind segment_batch_device: chunk k's GrabCut lane starts as soon as chunk k's trimaps are
        on the device; the caller's stream goes on with chunk k+1's SLIC / graph / network / trimap.  plan: the call's
        _OutputPlan; each lane runs the output stage for its chunk."""
        import torch
        from concurrent.futures import ThreadPoolExecutor
        from ._engine import merge_graphs
        eng = self._eng
        dev = eng.device
        b, h, w, _ = bgr.shape
        n = len(chunks)
        cs = plan.color_space
        caller = torch.cuda.current_stream(dev)
        lanes = eng.lanes(n)
        if getattr(self, "_chunk_pool", None) is None or self._chunk_pool._max_workers != n:
            if getattr(self, "_chunk_pool", None) is not None:
                self._chunk_pool.shutdown(wait=True)
            self._chunk_pool = ThreadPoolExecutor(max_workers=n, thread_name_prefix="ggc-chunk")
        seg = eng.empty(b, h, w, dtype=torch.int32)
        trimap = eng.empty(b, h, w, dtype=torch.uint8)
        mask = eng.empty(b, h, w, dtype=torch.uint8)
        stage = _OutputStage(eng, plan, bgr, full_bgr)
        state = None
        if return_state:
            state = dict(gc_binary=eng.empty(b, h, w, dtype=torch.uint8), bgd=eng.empty(b, 65, dtype=torch.float64),
                         fgd=eng.empty(b, 65, dtype=torch.float64),
                         gc_image=bgr if cs == "rgb" else eng.empty(b, h, w, 3, dtype=torch.uint8))
        n_iter, seed = self.gc_config.n_iter, self.gc_config.seed
        t_host = time.perf_counter()
        stamps = []                                   # per chunk: events around its front stages / its lane's work

        def lane_work(k, lo, hi, ready, ev):
            leng, stream = lanes[k]
            torch.cuda.set_device(dev)
            with torch.cuda.stream(stream):
                stream.wait_event(ready)              # the chunk's trimap, written on the caller's stream
                if ev is not None:
                    ev[0].record(stream)
                img = bgr[lo:hi]
                gc_img = img if cs == "rgb" else leng.convert_color8(img, cs)
                m = mask[lo:hi]
                binary, _, bgd, fgd = leng.grabcut(gc_img, m, n_iter, 0, None, seed + lo)
                if refine_iters > 0:
                    binary, _, bgd, fgd = leng.grabcut(gc_img, m, refine_iters, 2, None, seed + lo, bgd, fgd)
                if return_state:
                    state["gc_binary"][lo:hi].copy_(binary)
                    state["bgd"][lo:hi].copy_(bgd)
                    state["fgd"][lo:hi].copy_(fgd)
                    if cs != "rgb":
                        state["gc_image"][lo:hi].copy_(gc_img)
                if ev is not None:
                    ev[1].record(stream)
                stage.run(leng, lo, hi, binary)
                if ev is not None:
                    ev[2].record(stream)
                done = torch.cuda.Event()
                done.record(stream)
            return done

        futures, parts = [], []
        for k, (lo, hi) in enumerate(chunks):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if timing is not None else None
            if ev is not None:
                ev[3].record(caller)
            s_k, g_k, p_k, t_k = self._front(eng, bgr[lo:hi], threshold_fg, threshold_bg, edge_aware, filter_radius,
                                             hints=None if hints is None else hints.chunk(lo, hi))
            seg[lo:hi].copy_(s_k)
            trimap[lo:hi].copy_(t_k)
            mask[lo:hi].copy_(t_k)
            if ev is not None:
                ev[4].record(caller)
            ready = torch.cuda.Event()
            ready.record(caller)
            parts.append((g_k, p_k))
            stamps.append(ev)
            futures.append(self._chunk_pool.submit(lane_work, k, lo, hi, ready, ev))
        graphs = merge_graphs([g for g, _ in parts], seg)            # under the lanes' GrabCut
        probs = torch.cat([p for _, p in parts])
        for f in futures:
            caller.wait_event(f.result())             # whatever the caller enqueues next sees the lanes' outputs
        out = stage.result(trimap, seg, graphs, probs, mask, state)
        if timing is not None:                        # stage times from stream events (the stages overlap: they add up to more than the wall time)
            torch.cuda.synchronize(dev)
            front = sum(e[3].elapsed_time(e[4]) for e in stamps) / 1e3
            timing["graph_build"], timing["data_prep"], timing["gcn_inference"] = front, 0.0, 0.0
            timing["grabcut"] = sum(e[0].elapsed_time(e[1]) for e in stamps) / 1e3
            timing["postprocess"] = sum(e[1].elapsed_time(e[2]) for e in stamps) / 1e3
            timing["wall"] = time.perf_counter() - t_host
        return out

    def segment_batch(self, images: Sequence[np.ndarray], hints=None, full_images=None, strokes=None, polygons=None,
                      scissors=None, wands=None, **kwargs) -> list[SegmentationResult]:
        """Segment equally sized BGR images as one batch (additive API).  hints: one None or (fg_points, bg_points) per
        image, with hint_radius / hint_region / hints_as_prior / geodesic among kwargs (segment_batch_device).  strokes:
        one None or (fg_strokes, bg_strokes) per image, with stroke_radius among kwargs (segment_batch_device).  polygons:
        one None or (fg_polygons, bg_polygons, lassos) per image (segment_batch_device).  scissors: one None, anchor list
        or sequence of anchor lists per image, with scissors_options among kwargs (segment_batch_device).  wands: one None
        or (fg_points, bg_points) of magic-wand seeds per image, with wand=Wand(...) among kwargs (segment_batch_device).
        full_images
        (additive): the same images at one larger size each, (H1, W1, 3) uint8 BGR; every result's `full` then holds the
        outputs at that size (segment_batch_device's full_bgr).  foreground=True | ForegroundColours(...) among kwargs
        (with a matte) fills every result's foreground and rgba_clean.  full_cut=True | FullCut(...) among kwargs (with
        full_images) makes every result's full binary_mask, overlay and rgba those of cut_mask_full."""
        imgs = [_check_image(im) for im in images]
        if not imgs:
            return []
        if any(im.shape != imgs[0].shape for im in imgs):
            raise ValueError("segment_batch needs images of one size; group them by shape")
        _OutputPlan.of(self, (len(imgs), *imgs[0].shape), None if full_images is None else True,   # options before the list
                       **{k: kwargs[k] for k in _PLAN_OPTIONS if k in kwargs})
        full_bgr = None
        if full_images is not None:
            fulls = [_check_image(im) for im in full_images]
            if len(fulls) != len(imgs):
                raise ValueError(f"{len(fulls)} full images for {len(imgs)} images")
            if any(f.shape != fulls[0].shape for f in fulls):
                raise ValueError("segment_batch needs full images of one size; group them by shape")
            from ._engine import check_upsample_shapes
            check_upsample_shapes((len(imgs), *imgs[0].shape), (len(imgs), *imgs[0].shape[:2]),
                                  (len(imgs), *fulls[0].shape), "full_images")
            full_bgr = self._eng.to_device(np.stack(fulls))
        timing: dict[str, float] = {}
        bgr = self._eng.to_device(np.stack(imgs))
        if strokes is not None:
            kwargs["strokes"] = strokes
        if polygons is not None:
            kwargs["polygons"] = polygons
        if scissors is not None:
            kwargs["scissors"] = scissors
        if wands is not None:
            kwargs["wands"] = wands
        out = self.segment_batch_device(bgr, timing=timing, hints=hints, full_bgr=full_bgr, **kwargs)
        out.update({k: out[k].cpu() for k in _REFERENCE_FIELDS + _ADDITIVE_FIELDS if k in out})      # one copy per output, not one per image
        per_image = {k: v / len(imgs) for k, v in timing.items()}
        return [_result(out, i, imgs[i], dict(per_image)) for i in range(len(imgs))]

    def _click_round(self, binary, gt, mask, image, bgd, fgd, hint_ptr, hint_radius=5, n_iter=1):
        """One round of the NoC protocol on a device-resident batch: the next click per image on GrabCut's binary mask,
        painted into the mask as one hint per image (hint_ptr = arange(B+1); an image without a click has row -1, which
        ggc_apply_hints ignores), GC_EVAL for n_iter iterations from the kept models, IoU.
        -> (click (B,4) int32, binary, mask, bgd, fgd, iou (B,) float64), all on the device."""
        click = self._eng.next_click(binary, gt)
        self._eng.apply_hints(mask, click[:, :3].contiguous(), hint_ptr, hint_radius)
        return self._click_cut(click, binary, gt, mask, image, bgd, fgd, n_iter)

    def _click_round_geodesic(self, binary, gt, mask, image, bgd, fgd, bgr, clicks_dev, idx_dev, k, hint_ptr, geodesic, n_iter=1):
        """_click_round with geodesic hints: the new click is recorded first, then ALL k clicks made so far on each image
        are painted (clicks_dev[idx, :k, :3]: exactly k rows per image, rows of -1 are out of frame and ignored, so
        hint_ptr = arange(n+1) * k), so that an earlier click of the other label bounds the new one's reach."""
        eng = self._eng
        click = eng.next_click(binary, gt)
        clicks_dev[idx_dev, k - 1] = click
        rows = clicks_dev[idx_dev, :k, :3].reshape(-1, 3).contiguous()
        eng.geodesic_hints(bgr, rows, hint_ptr, geodesic.radius, geodesic.gamma, mask=mask)
        return self._click_cut(click, binary, gt, mask, image, bgd, fgd, n_iter)

    def _click_cut(self, click, binary, gt, mask, image, bgd, fgd, n_iter):
        """The end of a click round: GC_EVAL for n_iter iterations from the kept models on the painted mask, then IoU."""
        eng = self._eng
        binary, mask, bgd, fgd = eng.grabcut_lanes(image, mask, n_iter, 2, self.gc_config.seed, self._lane_count(binary.size(0)),
                                                   bgd, fgd)
        return (click, binary, mask, bgd, fgd, eng.iou(binary, gt)[0])

    def evaluate_clicks(self, images: Sequence[np.ndarray], gt_masks: Sequence[np.ndarray], max_clicks: int = 20,
                        iou_targets=(0.85, 0.90), hint_radius: int = 5, iters_per_click: int = 1,
                        stop_iou: Optional[float] = None, return_masks: bool = False, geodesic=False) -> dict:
        """Click guidance scored by the standard NoC protocol (additive), for equally sized BGR images and their ground
        truth (H,W) masks (nonzero = foreground).

        The automatic pipeline runs once; then, max_clicks times, a simulated user clicks the centre of the largest error
        region of every image (ggc_next_click), the click is painted as a disk of hint_radius pixels (ggc_apply_hints) and
        GrabCut continues in GC_EVAL mode for iters_per_click iterations from the kept mask and colour models; IoU is
        measured after each click (ggc_mask_iou).  Everything is scored on GrabCut's own binary mask, not on the
        clean_mask output of segment(): clean_mask can delete a clicked component, and the simulated user would then click
        the same place again and again.  With stop_iou, an image whose IoU reaches it gets no further clicks and its
        results stay frozen (the others continue as a compacted batch; a click round does not depend on an image's
        position in the batch, so every image gets what a one-image loop gives it).  The loop stays on the device: per
        round the host reads only ggc_apply_hints' hint_ptr and the IoU vector.  geodesic=True or GeodesicHints(...)
        (additive) paints by ggc_geodesic_hints instead of disks: every round passes all the clicks made so far on each
        active image, guided by the BGR images, which stay on the device; hint_radius is then ignored.

        Returns {"clicks": per image a list of (row, col, label) with label 1 = foreground, "ious": (B, max_clicks + 1)
        float64 (IoU after 0..max_clicks clicks; a stopped image repeats its last value), "noc": {t: (B,) int},
        "nof": {t: int}, "mean_iou": (max_clicks + 1,)} (metrics.noc_summary), and with return_masks=True "masks":
        (B, max_clicks + 1, H, W) uint8, GrabCut's label mask after each click."""
        import torch
        from .metrics import noc_summary
        imgs = [_check_image(im) for im in images]
        if not imgs:
            raise ValueError("evaluate_clicks needs at least one image")
        if any(im.shape != imgs[0].shape for im in imgs):
            raise ValueError("evaluate_clicks needs images of one size; group them by shape")
        gts = [np.asarray(g) for g in gt_masks]
        if len(gts) != len(imgs):
            raise ValueError(f"{len(gts)} ground-truth masks for {len(imgs)} images")
        if any(g.shape != imgs[0].shape[:2] for g in gts):
            raise ValueError(f"every ground-truth mask must be {imgs[0].shape[:2]} like its image")
        max_clicks, iters_per_click = int(max_clicks), int(iters_per_click)
        if max_clicks < 0 or iters_per_click < 1 or int(hint_radius) < 0:
            raise ValueError("max_clicks >= 0, iters_per_click >= 1 and hint_radius >= 0 are required")
        geo = _geodesic_args(geodesic)
        eng = self._eng
        b = len(imgs)
        gt = eng.to_device(np.stack([(g != 0) for g in gts]).astype(np.uint8))
        bgr = eng.to_device(np.stack(imgs))
        out = self.segment_batch_device(bgr, compose=False, return_state=True)
        if geo is None:
            bgr = None
        binary, mask, bgd, fgd, image = out["gc_binary"], out["gc_mask"], out["bgd"], out["fgd"], out["gc_image"]
        ious = np.zeros((b, max_clicks + 1))
        ious[:, 0] = eng.iou(binary, gt)[0].cpu().numpy()
        clicks_dev = torch.full((b, max(max_clicks, 1), 4), -1, dtype=torch.int32, device=eng.device)
        masks = None
        if return_masks:
            masks = eng.empty(b, max_clicks + 1, *binary.shape[1:], dtype=torch.uint8)
            masks[:, 0] = mask
        active = np.arange(b)                              # images still being clicked, in batch order
        idx_dev = torch.arange(b, device=eng.device)

        def compact(keep):
            nonlocal active, idx_dev, binary, mask, bgd, fgd, image, gt, bgr
            sel = torch.from_numpy(np.nonzero(keep)[0]).to(eng.device)
            active = active[keep]
            idx_dev, binary, mask, gt = (t.index_select(0, sel) for t in (idx_dev, binary, mask, gt))
            bgd, fgd, image = (t.index_select(0, sel) for t in (bgd, fgd, image))
            if bgr is not None:
                bgr = bgr.index_select(0, sel)

        if stop_iou is not None and (ious[:, 0] >= stop_iou).any():
            compact(ious[:, 0] < stop_iou)
        ptrs: dict[int, "torch.Tensor"] = {}
        for k in range(1, max_clicks + 1):
            ious[:, k] = ious[:, k - 1]                     # frozen unless the image is still active
            if masks is not None:
                masks[:, k] = masks[:, k - 1]
            if len(active) == 0:
                continue
            n = len(active)
            if n not in ptrs:
                ptrs[n] = torch.arange(n + 1, dtype=torch.int32, device=eng.device)
            if geo is not None:
                click, binary, mask, bgd, fgd, iou = self._click_round_geodesic(
                    binary, gt, mask, image, bgd, fgd, bgr, clicks_dev, idx_dev, k, ptrs[n] * k, geo, iters_per_click)
            else:
                click, binary, mask, bgd, fgd, iou = self._click_round(binary, gt, mask, image, bgd, fgd, ptrs[n], hint_radius,
                                                                       iters_per_click)
                clicks_dev[idx_dev, k - 1] = click
            ious[active, k] = iou.cpu().numpy()
            if masks is not None:
                masks[idx_dev, k] = mask
            if stop_iou is not None and (ious[active, k] >= stop_iou).any():
                compact(ious[active, k] < stop_iou)
        host_clicks = clicks_dev.cpu().numpy()
        clicks = [[(int(r), int(c), int(l)) for r, c, l, _ in host_clicks[i, :max_clicks] if r >= 0] for i in range(b)]
        res = {"clicks": clicks, "ious": ious}
        res.update(noc_summary(ious, iou_targets, max_clicks))
        if masks is not None:
            res["masks"] = masks.cpu().numpy()
        return res

    # ------------------------------------------------------------ reference API
    def segment(self, image: np.ndarray, threshold_fg: float = 0.55, threshold_bg: float = 0.55,
                refine_iters: int = 0, min_area_ratio: float = 0.002, keep_largest: bool = False,
                edge_aware: bool = True, filter_radius: int = 8, fg_points=None, bg_points=None, hint_radius: int = 5,
                hint_region: bool = False, hints_as_prior: bool = False, matte: bool = False,
                matte_radius: int = MATTE_RADIUS, matte_eps: float = MATTE_EPS,
                full_image: Optional[np.ndarray] = None, foreground=False, full_cut=False,
                geodesic=False, fg_strokes=None, bg_strokes=None, stroke_radius: int = 3,
                lasso=None, fg_polygons=None, bg_polygons=None, scissors=None,
                scissors_options: Optional[Scissors] = None, fg_wand=None, bg_wand=None,
                wand: Optional[Wand] = None) -> SegmentationResult:
        """Full pipeline on one BGR image (reference pipeline.py:265-352).

        Additive: fg_points / bg_points are user clicks, (row, col) pairs, applied as hard constraints on the trimap
        GrabCut starts from (see segment_batch_device for hint_radius, hint_region and hints_as_prior); matte=True also
        fills the result's alpha and rgba_soft (segment_batch_device), matte=ClosedFormMatte(...) with the closed-form
        matte; full_image, the same image at a larger size, fills
        the result's `full` (segment_batch_device's full_bgr; with matte=ClosedFormMatte(full_resolution=True) its
        alpha, rgba_soft and binary_mask come from closed_form_matte_full); foreground=True | ForegroundColours(...),
        with a matte, fills the result's foreground and rgba_clean (estimate_foreground under that matte's alpha);
        full_cut=True | FullCut(...), with full_image, makes the full binary_mask, overlay and rgba those of
        cut_mask_full of the cleaned mask (segment_batch_device); geodesic=True | GeodesicHints(...) paints the clicks by
        their geodesic distance on the image instead of disks (hint_radius is then ignored; segment_batch_device);
        fg_strokes / bg_strokes are brush strokes, sequences of polylines of (row, col) vertices, painted with
        stroke_radius as hard constraints before the clicks (segment_batch_device's strokes); lasso, one polygon or a
        sequence of polygons of (row, col) vertices, makes everything outside all of them definite background, and
        fg_polygons / bg_polygons are filled areas of definite labels, all before strokes and clicks
        (segment_batch_device's polygons); scissors, one list of (row, col) anchors on the object's outline or a
        sequence of such lists, is traced along the image's edges into closed outlines that join the lassos
        (intelligent scissors with scissors_options, a Scissors; segment_batch_device's scissors); fg_wand / bg_wand are
        magic-wand seeds, (row, col) pairs: what each selects on the image with `wand` (a Wand; None: its defaults)
        becomes definite foreground / background, after the polygons and before strokes and clicks
        (segment_batch_device's wands)."""
        image = _check_image(image)
        full = None if full_image is None else _check_image(full_image)
        _OutputPlan.of(self, (1, *image.shape), None if full is None else (1, *full.shape), min_area_ratio=min_area_ratio,
                       keep_largest=keep_largest, matte=matte, matte_radius=matte_radius, matte_eps=matte_eps,
                       foreground=foreground, full_cut=full_cut, geodesic=geodesic, hint_region=hint_region)
        full_bgr = None if full is None else self._eng.to_device(full[None])
        timing: dict[str, float] = {}
        hints = None if fg_points is None and bg_points is None else \
            [(() if fg_points is None else fg_points, () if bg_points is None else bg_points)]
        strokes = None if fg_strokes is None and bg_strokes is None else \
            [(() if fg_strokes is None else fg_strokes, () if bg_strokes is None else bg_strokes)]
        polygons = None if lasso is None and fg_polygons is None and bg_polygons is None else \
            [(() if fg_polygons is None else fg_polygons, () if bg_polygons is None else bg_polygons, lasso_list(lasso))]
        wands = None if fg_wand is None and bg_wand is None else \
            [(() if fg_wand is None else fg_wand, () if bg_wand is None else bg_wand)]
        out = self.segment_batch_device(self._eng.to_device(image[None]), threshold_fg, threshold_bg, refine_iters,
                                        min_area_ratio, keep_largest, edge_aware, filter_radius, timing=timing,
                                        hints=hints, hint_radius=hint_radius, hint_region=hint_region,
                                        hints_as_prior=hints_as_prior, matte=matte, matte_radius=matte_radius,
                                        matte_eps=matte_eps, full_bgr=full_bgr, foreground=foreground, full_cut=full_cut,
                                        geodesic=geodesic, strokes=strokes, stroke_radius=stroke_radius, polygons=polygons,
                                        scissors=None if scissors is None else [scissors], scissors_options=scissors_options,
                                        wands=wands, wand=wand)
        return _result(out, 0, image, timing)

    def segment_bbox(self, image: np.ndarray, bbox: tuple[int, int, int, int], matte: bool = False,
                     matte_radius: int = MATTE_RADIUS, matte_eps: float = MATTE_EPS,
                     full_image: Optional[np.ndarray] = None, foreground=False, full_cut=False) -> SegmentationResult:
        """Classical GrabCut with a bounding box (reference pipeline.py:354-380).  Additive: matte=True also fills the
        result's alpha and rgba_soft, the soft matte of the returned mask (alpha_matte; closed_form_matte with
        matte=ClosedFormMatte(...)); full_image, the same image at a
        larger size, fills the result's `full` from the returned mask (upsample_mask, then the overlay and cut-out;
        closed_form_matte_full with matte=ClosedFormMatte(full_resolution=True));
        foreground=True | ForegroundColours(...), with a matte, fills the result's foreground and rgba_clean;
        full_cut=True | FullCut(...), with full_image, makes the full binary_mask cut_mask_full of the returned mask
        (GrabCutConfig's colour space and seed, clean_mask's defaults)."""
        image = _check_image(image)
        full = None if full_image is None else _check_image(full_image)
        plan = _OutputPlan.of(self, (1, *image.shape), None if full is None else (1, *full.shape), matte=matte,
                              matte_radius=matte_radius, matte_eps=matte_eps, foreground=foreground, full_cut=full_cut)
        gc = GrabCut(image, self.gc_config, device=self.device)
        binary_mask = gc.run_with_bbox(bbox)
        x, y, w, h = bbox
        H, W = image.shape[:2]
        trimap = np.full((H, W), Label.BG_PROBABLE, dtype=np.uint8)
        trimap[y:y + h, x:x + w] = Label.FG_PROBABLE
        y0, y1, x0, x1 = eroded_box(H, W, bbox)
        if y1 > y0 and x1 > x0:
            trimap[y0:y1, x0:x1] = Label.FG_DEFINITE
        extra = {}
        if plan.mat or plan.cfm or full is not None:   # GrabCut's mask is final: no clean-up, and the overlay is GrabCut's own
            eng = self._eng
            stage = _OutputStage(eng, plan, eng.to_device(image[None]), None if full is None else eng.to_device(full[None]),
                                 final_mask=eng.to_device(np.ascontiguousarray(binary_mask, np.uint8)[None]))
            stage.from_mask(eng, 0, 1)
            extra = _optional_results(stage.out, 0)
        return SegmentationResult(image=image, binary_mask=binary_mask, trimap=trimap,
                                  segments=np.zeros((H, W), dtype=np.int32), overlay=gc.overlay_mask(),
                                  rgba=gc.crop_foreground(), **extra)

    def segment_scissors(self, image: np.ndarray, anchors, scissors_options: Optional[Scissors] = None,
                         **kwargs) -> SegmentationResult:
        """Classical GrabCut from a few anchors on the object's outline (additive; the sibling of segment_lasso, no
        network).  anchors: one list of (row, col) anchors or a sequence of such lists; each is traced
        into a closed outline by intelligent scissors (trace_boundary with scissors_options) on the BGR image, and the
        outlines are segment_lasso's polygons (GrabCut.run_with_lasso).  kwargs are segment_lasso's."""
        image = _check_image(image)
        traced = _trace_closed(self._eng, self._eng.to_device(image[None]), [anchors], _scissors_args(scissors_options))[0]
        if not traced:
            raise ValueError("segment_scissors needs at least one anchor list")
        return self.segment_lasso(image, traced, **kwargs)

    def segment_wand(self, image: np.ndarray, bg_points, fg_points=(), wand: Optional[Wand] = None, matte: bool = False,
                     matte_radius: int = MATTE_RADIUS, matte_eps: float = MATTE_EPS, full_image: Optional[np.ndarray] = None,
                     foreground=False, full_cut=False) -> SegmentationResult:
        """Classical GrabCut from magic-wand seeds (additive; the sibling of segment_lasso, no network).
        bg_points: (row, col) seeds on the backdrop; fg_points: optional seeds on the object.  The mask starts as definite
        background on what the background seeds select, definite foreground on what the foreground seeds select and
        probable foreground elsewhere (GrabCut.run_with_wand: ggc_wand_select, then run_with_trimap).  A ValueError if
        no pixel is selected as background, or every pixel is.  The optional matte / full-image arguments are
        segment_bbox's."""
        image = _check_image(image)
        full = None if full_image is None else _check_image(full_image)
        plan = _OutputPlan.of(self, (1, *image.shape), None if full is None else (1, *full.shape), matte=matte,
                              matte_radius=matte_radius, matte_eps=matte_eps, foreground=foreground, full_cut=full_cut)
        gc = GrabCut(image, self.gc_config, device=self.device)
        trimap = gc.wand_trimap(bg_points, fg_points, wand)
        binary_mask = gc.run_with_trimap(trimap)
        H, W = image.shape[:2]
        extra = {}
        if plan.mat or plan.cfm or full is not None:   # GrabCut's mask is final, as in segment_bbox
            eng = self._eng
            stage = _OutputStage(eng, plan, eng.to_device(image[None]), None if full is None else eng.to_device(full[None]),
                                 final_mask=eng.to_device(np.ascontiguousarray(binary_mask, np.uint8)[None]))
            stage.from_mask(eng, 0, 1)
            extra = _optional_results(stage.out, 0)
        return SegmentationResult(image=image, binary_mask=binary_mask, trimap=trimap,
                                  segments=np.zeros((H, W), dtype=np.int32), overlay=gc.overlay_mask(),
                                  rgba=gc.crop_foreground(), **extra)

    def segment_lasso(self, image: np.ndarray, polygon, matte: bool = False, matte_radius: int = MATTE_RADIUS,
                      matte_eps: float = MATTE_EPS, full_image: Optional[np.ndarray] = None, foreground=False,
                      full_cut=False) -> SegmentationResult:
        """Classical GrabCut with a lasso (additive; the sibling of segment_bbox, no network).  polygon:
        one polygon, a sequence of n >= 3 (row, col) vertices, or a sequence of polygons (their union).  The mask starts
        as probable foreground inside the lasso and definite background outside (GrabCut.run_with_lasso: ggc_apply_polygons,
        then run_with_trimap).  The optional matte / full-image arguments are segment_bbox's.  Not promised to equal
        segment_bbox on a rectangle: run_with_trimap applies the promotions and the degenerate guard, run_with_bbox does
        not."""
        image = _check_image(image)
        full = None if full_image is None else _check_image(full_image)
        plan = _OutputPlan.of(self, (1, *image.shape), None if full is None else (1, *full.shape), matte=matte,
                              matte_radius=matte_radius, matte_eps=matte_eps, foreground=foreground, full_cut=full_cut)
        gc = GrabCut(image, self.gc_config, device=self.device)
        trimap = gc.lasso_trimap(polygon)
        binary_mask = gc.run_with_trimap(trimap)
        H, W = image.shape[:2]
        extra = {}
        if plan.mat or plan.cfm or full is not None:   # GrabCut's mask is final, as in segment_bbox
            eng = self._eng
            stage = _OutputStage(eng, plan, eng.to_device(image[None]), None if full is None else eng.to_device(full[None]),
                                 final_mask=eng.to_device(np.ascontiguousarray(binary_mask, np.uint8)[None]))
            stage.from_mask(eng, 0, 1)
            extra = _optional_results(stage.out, 0)
        return SegmentationResult(image=image, binary_mask=binary_mask, trimap=trimap,
                                  segments=np.zeros((H, W), dtype=np.int32), overlay=gc.overlay_mask(),
                                  rgba=gc.crop_foreground(), **extra)
