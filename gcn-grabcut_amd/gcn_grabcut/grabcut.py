"""
GrabCut — host mirror of reference src/gcn_grabcut/grabcut.py.

Same class and method names; cv2.grabCut is replaced by ggc_grabcut in
libggc_hip.so (GMM colour models + push-relabel min-cut on the 8-neighbour
pixel grid, on the MI355X).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from enum import IntEnum
from typing import List, Optional, Tuple

import numpy as np


class Label(IntEnum):
    """Pixel label constants — OpenCV GrabCut convention (reference grabcut.py:22-27)."""
    BG_DEFINITE = 0   # cv2.GC_BGD
    FG_DEFINITE = 1   # cv2.GC_FGD
    BG_PROBABLE = 2   # cv2.GC_PR_BGD
    FG_PROBABLE = 3   # cv2.GC_PR_FGD


@dataclass
class GrabCutConfig:
    """reference grabcut.py:30-35.  As in the reference, only n_iter and color_space
    take effect (gamma and n_components are fixed at OpenCV's 50 and 5)."""
    n_iter: int = 5
    n_components: int = 5
    gamma: float = 50.0
    color_space: str = "rgb"   # "rgb" | "hsv" | "lab"
    seed: int = 0              # additive: seed of the k-means++ GMM initialisation


@dataclass
class GrabCutSnapshot:
    """State snapshot captured after each GrabCut run."""
    tag: str
    fg_pixels: int
    bg_pixels: int
    fg_ratio: float
    mask_copy: np.ndarray = field(repr=False)


class GrabCut:
    """
    gc = GrabCut(image)
    mask = gc.run_with_bbox((x, y, w, h))    # classical mode
    mask = gc.run_with_trimap(trimap)        # GCN-guided mode
    mask = gc.run_with_lasso(polygon)        # classical mode from a closed outline (additive)
    gc.add_hints(fg_points=[(r, c)])         # user clicks as definite labels (additive) ...
    mask = gc.refine(2)                      # ... then GC_EVAL from the edited mask
    """

    def __init__(self, image: np.ndarray, config: Optional[GrabCutConfig] = None, device="cuda"):
        from ._engine import get_engine
        if not isinstance(image, np.ndarray) or image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8:
            raise ValueError("image must be a BGR uint8 array of shape (H, W, 3)")
        self.image = image
        self.config = config or GrabCutConfig()
        self.mask: Optional[np.ndarray] = None
        self._dmask = None                     # (1,H,W) device copy of mask as the last run / edit left it
        self._bgd = np.zeros((1, 65), np.float64)
        self._fgd = np.zeros((1, 65), np.float64)
        self.history: List[GrabCutSnapshot] = []
        self._eng = get_engine(device)
        self._proc = self._preprocess(image)

    def _preprocess(self, image: np.ndarray):
        """BGR uint8 -> the (1,H,W,3) uint8 device image GrabCut works on (reference grabcut.py:73-79).  hsv / lab are
        8-bit conversions in the style of cv2.cvtColor (ggc_convert_color8; parity with OpenCV unpinned)."""
        cs = self.config.color_space.lower()
        dev = self._eng.to_device(np.ascontiguousarray(image)[None])
        if cs in ("hsv", "lab"):
            return self._eng.convert_color8(dev, cs)
        if cs != "rgb":
            raise ValueError(f"unknown color_space '{cs}': rgb | hsv | lab")
        return dev

    def _run(self, mask: Optional[np.ndarray], n_iter: int, mode: int, rect=None) -> np.ndarray:
        import torch
        eng = self._eng
        h, w = self.image.shape[:2]
        dmask = eng.to_device(mask[None]) if mask is not None else torch.zeros(1, h, w, dtype=torch.uint8, device=eng.device)
        bgd, fgd = eng.to_device(self._bgd), eng.to_device(self._fgd)
        _, dmask, bgd, fgd = eng.grabcut(self._proc, dmask, n_iter, mode, None if rect is None else [list(rect)],
                                         self.config.seed, bgd, fgd)
        self.mask = dmask[0].cpu().numpy()
        self._dmask = dmask
        self._bgd, self._fgd = bgd.cpu().numpy(), fgd.cpu().numpy()
        return self._binary()

    def run_with_bbox(self, bbox: Tuple[int, int, int, int]) -> np.ndarray:
        """Classical GrabCut, bbox = (x, y, w, h) — reference grabcut.py:81-102."""
        self._bgd = np.zeros((1, 65), np.float64)
        self._fgd = np.zeros((1, 65), np.float64)
        out = self._run(None, self.config.n_iter, 1, bbox)
        self._snapshot("bbox_init")
        return out

    def run_with_trimap(self, trimap: np.ndarray) -> np.ndarray:
        """GCN-guided GrabCut seeded with a trimap in {0,1,2,3} — reference grabcut.py:104-151.
        The promotion of probable labels and the single-class guard run inside ggc_grabcut."""
        if trimap.shape != self.image.shape[:2]:
            raise ValueError(f"Trimap shape {trimap.shape} != image shape {self.image.shape[:2]}")
        if trimap.dtype != np.uint8:
            trimap = trimap.astype(np.uint8)
        self._bgd = np.zeros((1, 65), np.float64)
        self._fgd = np.zeros((1, 65), np.float64)
        out = self._run(np.ascontiguousarray(trimap), self.config.n_iter, 0)
        degenerate = not ((self.mask == Label.FG_DEFINITE).any() and (self.mask == Label.BG_DEFINITE).any())
        self._snapshot("trimap_degenerate" if degenerate else "trimap_init")
        return out

    def lasso_trimap(self, polygon) -> np.ndarray:
        """Additive: the start mask of run_with_lasso, GC_PR_FGD inside the lasso (one polygon of (row, col) vertices or a
        sequence of polygons, their union; boundary included) and GC_BGD outside (ggc_apply_polygons)."""
        from .graph_builder import pack_polygons, lasso_list
        lassos = lasso_list(polygon)
        if not lassos:
            raise ValueError("a lasso needs at least one polygon")
        eng = self._eng
        h, w = self.image.shape[:2]
        start = eng.to_device(np.full((1, h, w), Label.FG_PROBABLE, np.uint8))
        return eng.apply_polygons(start, *eng.upload_polygons(*pack_polygons([((), (), lassos)])))[0].cpu().numpy()

    def run_with_lasso(self, polygon) -> np.ndarray:
        """Additive: classical GrabCut from a lasso, the polygon sibling of run_with_bbox: lasso_trimap(polygon), then
        run_with_trimap (so the promotion of probable labels and the single-class guard apply)."""
        return self.run_with_trimap(self.lasso_trimap(polygon))

    def wand_trimap(self, bg_points, fg_points=(), wand=None) -> np.ndarray:
        """Additive: the start mask of run_with_wand: GC_BGD on what the background seeds' magic-wand selections hold on
        self.image, GC_FGD on the foreground seeds', GC_PR_FGD elsewhere (ggc_wand_select; `wand` is a pipeline.Wand,
        None: its defaults; background seeds come after foreground ones and win).  A ValueError if no pixel is decided
        as background, or every pixel is: GrabCut would have no background model, or nothing left to cut."""
        from .pipeline import _wand_args
        from .graph_builder import pack_hints
        wand = _wand_args(wand)
        rows, ptr = pack_hints([(fg_points if fg_points is not None else (), bg_points if bg_points is not None else ())])
        eng = self._eng
        h, w = self.image.shape[:2]
        n_bg = 0
        start = eng.to_device(np.full((1, h, w), Label.FG_PROBABLE, np.uint8))
        if ptr[-1]:
            d_rows, d_ptr = eng.upload_hints(rows, ptr)
            _, _, counts = eng.wand_select(eng.to_device(np.ascontiguousarray(self.image)[None]), d_rows, d_ptr, *wand.args(),
                                           mask=start, select=False, counts=True)
            n_bg = int(counts[0, 1].item())
        if n_bg == 0:
            raise ValueError("the wand selected no background pixel: give a background seed inside the image")
        if n_bg == h * w:
            raise ValueError("the wand selected every pixel as background: lower the tolerance or move the seed")
        return start[0].cpu().numpy()

    def run_with_wand(self, bg_points, fg_points=(), wand=None) -> np.ndarray:
        """Additive: classical GrabCut from magic-wand seeds, the sibling of run_with_lasso: wand_trimap(bg_points,
        fg_points, wand), then run_with_trimap (so the promotion of probable labels and the single-class guard apply)."""
        return self.run_with_trimap(self.wand_trimap(bg_points, fg_points, wand))

    def add_wand(self, fg_points=(), bg_points=(), wand=None) -> np.ndarray:
        """Additive: paint magic-wand selections into the current mask as GC_FGD / GC_BGD (ggc_wand_select on self.image;
        `wand` is a pipeline.Wand, None: its defaults; background seeds win where selections overlap).  The edit runs on
        the mask the last run left on the device; the GMMs are kept, so refine(n) continues from the edited mask, as
        after add_strokes."""
        if self.mask is None:
            raise RuntimeError("Call run_with_bbox or run_with_trimap first.")
        from .pipeline import _wand_args
        from .graph_builder import pack_hints
        wand = _wand_args(wand)
        rows, ptr = pack_hints([(fg_points, bg_points)])
        eng = self._eng
        if self._dmask is None or not self.history or not np.array_equal(self.mask, self.history[-1].mask_copy):
            self._dmask = eng.to_device(np.ascontiguousarray(self.mask, dtype=np.uint8)[None])   # the host mask was edited
        if ptr[-1]:
            d_rows, d_ptr = eng.upload_hints(rows, ptr)
            eng.wand_select(eng.to_device(np.ascontiguousarray(self.image)[None]), d_rows, d_ptr, *wand.args(),
                            mask=self._dmask, select=False)
            self.mask = self._dmask[0].cpu().numpy()
        self._snapshot("wand")
        return self._binary()

    def refine(self, extra_iter: int = 3) -> np.ndarray:
        """Continue from the current GMM state (GC_EVAL) — reference grabcut.py:153-163."""
        if self.mask is None:
            raise RuntimeError("Call run_with_bbox or run_with_trimap first.")
        out = self._run(self.mask, extra_iter, 2)
        self._snapshot("refinement")
        return out

    def add_hints(self, fg_points=(), bg_points=(), radius: int = 5, geodesic=False) -> np.ndarray:
        """Additive: paint user clicks, (row, col) pairs, into the current mask as GC_FGD / GC_BGD disks of `radius` pixels
        (ggc_apply_hints; background clicks win where disks overlap, clicks outside the image are ignored).  The edit runs
        on the mask the last run left on the device; the GMMs are kept, so refine(n) continues from the edited mask.
        geodesic=True or a pipeline.GeodesicHints paints by geodesic distance on self.image instead (ggc_geodesic_hints;
        `radius` is then ignored): only the clicks of this call bound each other's reach."""
        if self.mask is None:
            raise RuntimeError("Call run_with_bbox or run_with_trimap first.")
        if int(radius) < 0:
            raise ValueError(f"radius must be >= 0, got {radius}")
        from .pipeline import _geodesic_args
        geo = _geodesic_args(geodesic)
        from .graph_builder import pack_hints
        rows, ptr = pack_hints([(fg_points, bg_points)])
        eng = self._eng
        if self._dmask is None or not self.history or not np.array_equal(self.mask, self.history[-1].mask_copy):
            self._dmask = eng.to_device(np.ascontiguousarray(self.mask, dtype=np.uint8)[None])   # the host mask was edited
        if ptr[-1]:
            hints, hint_ptr = eng.upload_hints(rows, ptr)
            if geo is not None:
                eng.geodesic_hints(eng.to_device(np.ascontiguousarray(self.image)[None]), hints, hint_ptr, geo.radius, geo.gamma,
                                   mask=self._dmask)
            else:
                eng.apply_hints(self._dmask, hints, hint_ptr, radius)
            self.mask = self._dmask[0].cpu().numpy()
        self._snapshot("hints")
        return self._binary()

    def add_strokes(self, fg_strokes=(), bg_strokes=(), radius: int = 3, geodesic=False) -> np.ndarray:
        """Additive: paint brush strokes, polylines of (row, col) vertices, into the current mask as GC_FGD / GC_BGD within
        `radius` pixels of each stroke (ggc_apply_strokes; radius 0: the centre line; background strokes win where the two
        overlap; the part of a stroke inside the image is painted).  The edit runs on the mask the last run left on the
        device; the GMMs are kept, so refine(n) continues from the edited mask.  geodesic=True or a pipeline.GeodesicHints
        paints by geodesic distance on self.image from the strokes' centre-line pixels instead (ggc_stroke_pixels, then
        ggc_geodesic_hints; `radius` is then ignored)."""
        if self.mask is None:
            raise RuntimeError("Call run_with_bbox or run_with_trimap first.")
        from .pipeline import _geodesic_args, _check_stroke_radius
        radius = _check_stroke_radius(radius, "radius")
        geo = _geodesic_args(geodesic)
        from .graph_builder import pack_strokes
        segs, ptr = pack_strokes([(fg_strokes, bg_strokes)])
        eng = self._eng
        if self._dmask is None or not self.history or not np.array_equal(self.mask, self.history[-1].mask_copy):
            self._dmask = eng.to_device(np.ascontiguousarray(self.mask, dtype=np.uint8)[None])   # the host mask was edited
        if ptr[-1]:
            d_segs, d_ptr = eng.upload_strokes(segs, ptr)
            if geo is not None:
                rows, row_ptr = eng.stroke_pixels(tuple(self._dmask.shape), d_segs, d_ptr)
                eng.geodesic_hints(eng.to_device(np.ascontiguousarray(self.image)[None]), rows, row_ptr, geo.radius, geo.gamma,
                                   mask=self._dmask)
            else:
                eng.apply_strokes(self._dmask, d_segs, d_ptr, radius)
            self.mask = self._dmask[0].cpu().numpy()
        self._snapshot("strokes")
        return self._binary()

    def add_polygons(self, fg_polygons=(), bg_polygons=(), lasso=None) -> np.ndarray:
        """Additive: paint filled polygons and lassos into the current mask (ggc_apply_polygons): every pixel outside all
        lassos (one polygon or a sequence of them) becomes GC_BGD, then every pixel a fill covers GC_FGD / GC_BGD,
        background fills winning where the two overlap.  The edit runs on the mask the last run left on the device; the
        GMMs are kept, so refine(n) continues from the edited mask, as after add_strokes."""
        if self.mask is None:
            raise RuntimeError("Call run_with_bbox or run_with_trimap first.")
        from .graph_builder import pack_polygons, lasso_list
        packed = pack_polygons([(fg_polygons, bg_polygons, lasso_list(lasso))])
        eng = self._eng
        if self._dmask is None or not self.history or not np.array_equal(self.mask, self.history[-1].mask_copy):
            self._dmask = eng.to_device(np.ascontiguousarray(self.mask, dtype=np.uint8)[None])   # the host mask was edited
        if len(packed[2]):
            eng.apply_polygons(self._dmask, *eng.upload_polygons(*packed))
            self.mask = self._dmask[0].cpu().numpy()
        self._snapshot("polygons")
        return self._binary()

    def _binary(self) -> np.ndarray:
        return np.where((self.mask == Label.FG_DEFINITE) | (self.mask == Label.FG_PROBABLE), 1, 0).astype(np.uint8)

    def _snapshot(self, tag: str) -> None:
        b = self._binary()
        self.history.append(GrabCutSnapshot(tag=tag, fg_pixels=int(b.sum()), bg_pixels=int((b == 0).sum()),
                                            fg_ratio=float(b.mean()), mask_copy=self.mask.copy()))

    def _compose(self, alpha: float, color: Tuple):
        eng = self._eng
        binary = eng.to_device(self._binary()[None])
        return eng.compose(eng.to_device(np.ascontiguousarray(self.image)[None]), binary, alpha, tuple(color[::-1]))

    def overlay_mask(self, alpha: float = 0.45, color: Tuple = (0, 220, 100)) -> np.ndarray:
        """BGR image with a coloured foreground overlay — reference grabcut.py:180-188."""
        return self._compose(alpha, color)[0][0].cpu().numpy()

    def crop_foreground(self) -> np.ndarray:
        """BGRA image with the background transparent — reference grabcut.py:190-195."""
        return self._compose(0.45, (0, 220, 100))[1][0].cpu().numpy()

    def trimap_visualisation(self, trimap: np.ndarray) -> np.ndarray:
        vis = np.zeros((*trimap.shape, 3), dtype=np.uint8)
        vis[trimap == Label.BG_DEFINITE] = [0, 0, 0]
        vis[trimap == Label.FG_DEFINITE] = [255, 255, 255]
        vis[trimap == Label.BG_PROBABLE] = [80, 0, 0]
        vis[trimap == Label.FG_PROBABLE] = [0, 200, 200]
        return vis
