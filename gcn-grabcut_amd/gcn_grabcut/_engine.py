"""
Batched device engine: the hot path of GCNGrabCutPipeline.segment expressed as
calls into libggc_hip.so on tensors that stay in HBM.

Every public class of this package (GraphBuilder, GrabCut, refine_trimap, ...)
is a thin view over these methods with batch size 1; `segment_batch` uses them
with the whole batch.  PyTorch provides device memory and the stream only.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native


@dataclass
class DeviceGraphs:
    """Superpixel graphs of a batch, packed PyG-Batch style, resident in HBM."""
    segments: torch.Tensor      # (B,H,W) int32
    n_nodes: torch.Tensor       # (B,)   int32
    node_ptr_host: np.ndarray   # (B+1,) int64
    edge_ptr_host: np.ndarray   # (B+1,) int64
    node_ptr: torch.Tensor      # (B+1,) int32 on device
    x: torch.Tensor             # (N,19) float32 = 16 image features || 3 prior
    centroids: torch.Tensor     # (N,2)
    area_ratio: torch.Tensor    # (N,)
    edge_src: torch.Tensor      # (E,) int32, global ids
    edge_dst: torch.Tensor      # (E,) int32, global ids
    edge_attr: torch.Tensor     # (E,5)

    @property
    def batch_size(self) -> int:
        return self.segments.size(0)


class Engine:
    def __init__(self, device_index: int = 0, private_context: bool = False):
        if not torch.cuda.is_available():
            raise RuntimeError("gcn_grabcut needs an MI355X: no HIP device is visible and there is no CPU fallback")
        self.index = int(device_index)
        self.device = torch.device("cuda", self.index)
        # a private context owns its scratch arena, so it can run concurrently with the shared one on another stream
        self.ctx = _native.Context(self.index) if private_context else _native.get_context(self.index)
        self._lanes = None

    # ------------------------------------------------------------------ concurrent lanes
    def lanes(self, n: int):
        """n (engine, stream) pairs with private contexts for work that is independent per image.  GrabCut's
        max-flow ends in rounds with a handful of open images that are pure launch latency; running sub-batches
        on separate streams lets one sub-batch's tail overlap another's bandwidth-bound rounds.  The list only
        grows: streams keep their hardware queue, and two lanes that share a queue serialise."""
        if self._lanes is None:
            self._lanes = []
        while len(self._lanes) < n:
            self._lanes.append((Engine(self.index, private_context=True), torch.cuda.Stream(self.device)))
        return self._lanes[:n]

    def grabcut_lanes(self, image, mask, n_iter=5, mode=0, seed=0, n_lanes=4, bgd=None, fgd=None, post=None):
        """grabcut() on n_lanes contiguous sub-batches at once; same results (image b keeps seed + b).

        Sub-batch 0 runs on the caller's stream, the others on n_lanes - 1 streams of the engine.  HIP maps streams onto 4
        hardware queues by default (GPU_MAX_HW_QUEUES) and two lanes that share a queue serialise: the caller's stream plus
        three created ones are the four queues of a fresh process (53 ms per stage at batch 256); all four lanes on created
        streams are five streams on four queues (measured in round 3: 77 ms)."""
        from concurrent.futures import ThreadPoolExecutor
        b = image.size(0)
        n_lanes = max(1, min(int(n_lanes), b))
        # post(engine, lo, hi, binary[lo:hi]): per-image follow-up work (clean-up, composition) that a lane runs on its own
        # stream as soon as ITS sub-batch is cut, under the other lanes' tails, instead of after the slowest lane
        if n_lanes == 1:
            out = self.grabcut(image, mask, n_iter, mode, None, seed, bgd, fgd)
            if post is not None:
                post(self, 0, b, out[0])
            return out
        bounds = [b * i // n_lanes for i in range(n_lanes + 1)]
        if bgd is None:
            bgd = torch.zeros(b, 65, dtype=torch.float64, device=self.device)
        if fgd is None:
            fgd = torch.zeros(b, 65, dtype=torch.float64, device=self.device)
        binary = self.empty(b, *image.shape[1:3], dtype=torch.uint8)
        caller = torch.cuda.current_stream(self.device)
        lanes = self.lanes(n_lanes - 1)          # sub-batch 0 runs here, on the caller's stream and context

        def run(i):
            eng, stream = lanes[i - 1]
            lo, hi = bounds[i], bounds[i + 1]
            torch.cuda.set_device(self.device)
            stream.wait_stream(caller)
            with torch.cuda.stream(stream):
                out = eng.grabcut(image[lo:hi], mask[lo:hi], n_iter, mode, None, seed + lo, bgd[lo:hi], fgd[lo:hi])
                binary[lo:hi].copy_(out[0])
                if post is not None:
                    post(eng, lo, hi, binary[lo:hi])
            stream.synchronize()

        if getattr(self, "_pool", None) is None or self._pool._max_workers < n_lanes - 1:
            if getattr(self, "_pool", None) is not None:
                self._pool.shutdown(wait=True)
            self._pool = ThreadPoolExecutor(max_workers=n_lanes - 1, thread_name_prefix="ggc-lane")
        futures = [self._pool.submit(run, i) for i in range(1, n_lanes)]
        out = self.grabcut(image[:bounds[1]], mask[:bounds[1]], n_iter, mode, None, seed, bgd[:bounds[1]], fgd[:bounds[1]])
        binary[:bounds[1]].copy_(out[0])
        if post is not None:
            post(self, 0, bounds[1], binary[:bounds[1]])
        for f in futures:
            f.result()
        return binary, mask, bgd, fgd

    def all_contexts(self):
        return [self.ctx] + [e.ctx for e, _ in (self._lanes or [])]

    # ------------------------------------------------------------------ helpers
    def _stream(self) -> int:
        return _native.current_stream(self.index)

    def to_device(self, a, dtype=None) -> torch.Tensor:
        if torch.is_tensor(a):
            t = a
        else:
            t = torch.from_numpy(np.ascontiguousarray(a))
        if dtype is not None:
            t = t.to(dtype)
        return t.to(self.device, non_blocking=True).contiguous()

    def empty(self, *shape, dtype=torch.float32) -> torch.Tensor:
        return torch.empty(*shape, dtype=dtype, device=self.device)

    # ------------------------------------------------------------------ G0 / G1
    def preprocess(self, bgr: torch.Tensor):
        """bgr (B,H,W,3) uint8 -> lab, hsv (B,H,W,3) f32, gray, grad (B,H,W) f32."""
        b, h, w, _ = bgr.shape
        lab, hsv = self.empty(b, h, w, 3), self.empty(b, h, w, 3)
        gray, grad = self.empty(b, h, w), self.empty(b, h, w)
        self.ctx.call("ggc_preprocess", self._stream(), b, h, w, bgr.data_ptr(), lab.data_ptr(), hsv.data_ptr(),
                      gray.data_ptr(), grad.data_ptr())
        return lab, hsv, gray, grad

    def slic(self, image: torch.Tensor, n_segments: int, compactness: float = 10.0, sigma: float = 1.0,
             rescale_input: bool = True):
        b, h, w, _ = image.shape
        seg = self.empty(b, h, w, dtype=torch.int32)
        n = self.empty(b, dtype=torch.int32)
        self.ctx.call("ggc_slic", self._stream(), b, h, w, image.data_ptr(), int(n_segments), float(compactness),
                      float(sigma), int(bool(rescale_input)), seg.data_ptr(), n.data_ptr())
        return seg, n

    def slic_rgb(self, bgr: torch.Tensor, n_segments: int, compactness: float = 10.0, sigma: float = 1.0):
        """SuperpixelGraphConfig(use_lab=False): SLIC on rgb.astype(float), skimage's float64 path (reference graph_builder.py:177-179)."""
        b, h, w, _ = bgr.shape
        seg = self.empty(b, h, w, dtype=torch.int32)
        n = self.empty(b, dtype=torch.int32)
        self.ctx.call("ggc_slic_rgb", self._stream(), b, h, w, bgr.data_ptr(), int(n_segments), float(compactness), float(sigma),
                      seg.data_ptr(), n.data_ptr())
        return seg, n

    # ------------------------------------------------------------------ G2-G8
    def build_graphs(self, seg, n_nodes, lab, hsv, grad, connectivity: int = 4, n_nonlocal: int = 4) -> DeviceGraphs:
        b, h, w = seg.shape
        node_ptr = np.zeros(b + 1, np.int64)
        edge_ptr = np.zeros(b + 1, np.int64)
        self.ctx.call("ggc_graph_count", self._stream(), b, h, w, seg.data_ptr(), n_nodes.data_ptr(), lab.data_ptr(),
                      hsv.data_ptr(), grad.data_ptr(), int(connectivity), int(n_nonlocal), node_ptr.ctypes.data,
                      edge_ptr.ctypes.data)
        n, e = int(node_ptr[-1]), int(edge_ptr[-1])
        x, cen, area = self.empty(n, 19), self.empty(n, 2), self.empty(n)
        src = self.empty(max(e, 1), dtype=torch.int32)
        dst = self.empty(max(e, 1), dtype=torch.int32)
        attr = self.empty(max(e, 1), 5)
        self.ctx.call("ggc_graph_fill", self._stream(), x.data_ptr(), cen.data_ptr(), area.data_ptr(), src.data_ptr(),
                      dst.data_ptr(), attr.data_ptr(), 1)
        return DeviceGraphs(seg, n_nodes, node_ptr, edge_ptr, self.to_device(node_ptr.astype(np.int32)), x, cen, area,
                            src[:e], dst[:e], attr[:e])

    # ------------------------------------------------------------------ M0-M7
    def predict_probs(self, model, graphs: DeviceGraphs) -> torch.Tensor:
        from .data import Data
        d = Data(x=graphs.x, edge_attr=graphs.edge_attr)
        d.edge_index = torch.stack([graphs.edge_src, graphs.edge_dst]) if graphs.edge_src.numel() else \
            torch.zeros(2, 0, dtype=torch.int32, device=self.device)
        d.node_ptr32 = graphs.node_ptr
        return model.predict_probs_device(d, ctx=self.ctx)

    # ------------------------------------------------------------------ P0-P3, S0
    def refine_trimap(self, probs, node_ptr, seg, bgr, thr_fg=0.55, thr_bg=0.55, radius=8, eps=1e-3,
                      edge_aware=True) -> torch.Tensor:
        b, h, w = seg.shape
        tri = self.empty(b, h, w, dtype=torch.uint8)
        self.ctx.call("ggc_refine_trimap", self._stream(), b, h, w, probs.data_ptr(), node_ptr.data_ptr(),
                      seg.data_ptr(), bgr.data_ptr(), float(thr_fg), float(thr_bg), int(radius), float(eps),
                      int(bool(edge_aware)), tri.data_ptr())
        return tri

    def guided_filter(self, guide, src, radius=8, eps=1e-3) -> torch.Tensor:
        b, h, w = guide.shape
        out = self.empty(b, h, w)
        self.ctx.call("ggc_guided_filter", self._stream(), b, h, w, guide.data_ptr(), src.data_ptr(), int(radius),
                      float(eps), out.data_ptr())
        return out

    def seed_from_prior(self, trimap, prior, node_ptr, seg, seed_frac=0.1) -> torch.Tensor:
        b, h, w = seg.shape
        prior = prior.contiguous()
        self.ctx.call("ggc_seed_from_prior", self._stream(), b, h, w, prior.data_ptr(), node_ptr.data_ptr(),
                      seg.data_ptr(), float(seed_frac), trimap.data_ptr())
        return trimap

    # ------------------------------------------------------------------ H0
    def _upload_packed(self, arrays):
        """int32 host arrays -> their flat copies on the device, views of one buffer filled by one host-to-device copy."""
        parts = [np.asarray(a, np.int32).ravel() for a in arrays]
        d = self.to_device(np.concatenate(parts))
        o = np.cumsum([0] + [a.size for a in parts])
        return [d[o[i]:o[i + 1]] for i in range(len(parts))]

    def upload_hints(self, hints: np.ndarray, hint_ptr: np.ndarray):
        """pack_hints' (hints [K,3], hint_ptr [B+1]) -> the same two arrays on the device, in one host-to-device copy."""
        ptr, rows = self._upload_packed([hint_ptr, hints])
        return rows.view(-1, 3), ptr

    def apply_hints(self, mask, hints, hint_ptr, radius=5, region=False, segments=None, node_ptr=None, node_hints=None,
                    shape=None):
        """Clicks as hard constraints, in place on mask (B,H,W) uint8 (ggc_apply_hints).  node_hints (N,3) float32, if
        given, receives encode_user_hints of every image; mask may then be None, with shape = (B,H,W)."""
        b, h, w = mask.shape if mask is not None else shape
        self.ctx.call("ggc_apply_hints", self._stream(), b, h, w, _native.ptr(hints), hint_ptr.data_ptr(), int(radius),
                      int(bool(region)), _native.ptr(segments), _native.ptr(node_ptr), _native.ptr(node_hints),
                      _native.ptr(mask))
        return mask

    def geodesic_hints(self, bgr, hints, hint_ptr, radius=40, gamma=2, mask=None, segments=None, node_ptr=None,
                       dist_fg=None, dist_bg=None, node_dist=None):
        """Geodesic click hints (ggc_geodesic_hints, include/ggc.h H1): bgr (B,H,W,3) uint8 is the guide, hints / hint_ptr
        as for apply_hints.  mask (B,H,W) uint8 is painted in place; dist_fg / dist_bg (B,H,W) int32 and node_dist (N,2)
        int32 (with segments and node_ptr) receive the capped distances.  At least one output is needed."""
        b, h, w, _ = bgr.shape
        self.ctx.call("ggc_geodesic_hints", self._stream(), b, h, w, bgr.data_ptr(), _native.ptr(hints), hint_ptr.data_ptr(),
                      int(radius), int(gamma), _native.ptr(segments), _native.ptr(node_ptr), _native.ptr(mask),
                      _native.ptr(dist_fg), _native.ptr(dist_bg), _native.ptr(node_dist))
        return mask

    # ------------------------------------------------------------------ H2
    def upload_strokes(self, strokes: np.ndarray, stroke_ptr: np.ndarray):
        """pack_strokes' (strokes [S,5], stroke_ptr [B+1]) -> the same two arrays on the device, in one host-to-device copy."""
        ptr, rows = self._upload_packed([stroke_ptr, strokes])
        return rows.view(-1, 5), ptr

    def apply_strokes(self, mask, strokes, stroke_ptr, radius=3):
        """Brush strokes as hard constraints, in place on mask (B,H,W) uint8 (ggc_apply_strokes): strokes (S,5) int32 =
        r0, c0, r1, c1, label and stroke_ptr (B+1,) int32 on the device (upload_strokes)."""
        b, h, w = mask.shape
        self.ctx.call("ggc_apply_strokes", self._stream(), b, h, w, _native.ptr(strokes), stroke_ptr.data_ptr(), int(radius),
                      mask.data_ptr())
        return mask

    def stroke_pixels(self, shape, strokes, stroke_ptr):
        """The centre-line pixels of a batch's strokes as a click list (ggc_stroke_pixels): shape = (B,H,W) ->
        (hints (P,3) int32 = row, col, label; hint_ptr (B+1,) int32), both on the device.  One call counts, the next fills."""
        b, h, w = shape
        hint_ptr = self.empty(b + 1, dtype=torch.int32)
        args = (self._stream(), b, h, w, _native.ptr(strokes), stroke_ptr.data_ptr(), hint_ptr.data_ptr())
        self.ctx.call("ggc_stroke_pixels", *args, None, 0)
        n = int(hint_ptr[-1].item()) if b else 0
        hints = self.empty(n, 3, dtype=torch.int32)
        if n:
            self.ctx.call("ggc_stroke_pixels", *args, hints.data_ptr(), n)
        return hints, hint_ptr

    # ------------------------------------------------------------------ H3
    def upload_polygons(self, verts, poly_ptr, poly_label, image_ptr):
        """pack_polygons' (verts [V,2], poly_ptr [P+1], poly_label [P], image_ptr [B+1]) -> the same four arrays on the
        device, in one host-to-device copy."""
        ip, pp, pl, v = self._upload_packed([image_ptr, poly_ptr, poly_label, verts])
        return v.view(-1, 2), pp, pl, ip

    def apply_polygons(self, mask, verts, poly_ptr, poly_label, image_ptr):
        """Lassos and filled polygons as hard constraints, in place on mask (B,H,W) uint8 (ggc_apply_polygons): the four
        arrays of upload_polygons, on the device."""
        b, h, w = mask.shape
        self.ctx.call("ggc_apply_polygons", self._stream(), b, h, w, _native.ptr(verts), poly_ptr.data_ptr(),
                      _native.ptr(poly_label), image_ptr.data_ptr(), int(poly_label.numel()), mask.data_ptr())
        return mask

    # ------------------------------------------------------------------ H4
    def upload_paths(self, anchors, path_ptr, path_closed, image_ptr):
        """pack_paths' (anchors [A,2], path_ptr [Q+1], path_closed [Q], image_ptr [B+1]) -> the same four arrays on the
        device, in one host-to-device copy."""
        ip, pp, pc, a = self._upload_packed([image_ptr, path_ptr, path_closed, anchors])
        return a.view(-1, 2), pp, pc, ip

    def trace_paths(self, bgr, anchors, path_ptr, path_closed, image_ptr, margin=16, edge_cap=2048, smooth=16, capacity=0):
        """Intelligent scissors (ggc_trace_paths, include/ggc.h H4): bgr (B,H,W,3) uint8 is the guide, the four arrays
        of upload_paths on the device -> (verts (V,2) int32 = row, col; vert_ptr (Q+1,) int32), both on the device and
        in ggc_apply_polygons' packing.  capacity > 0 is a guess of V: the call fills a buffer of that many rows at once
        and is repeated only when the guess was too small (vert_ptr is written either way); 0: one call counts, the
        next fills."""
        b, h, w, _ = bgr.shape
        q = int(path_closed.numel())
        vert_ptr = torch.zeros(q + 1, dtype=torch.int32, device=self.device)
        if b == 0 or q == 0:
            return self.empty(0, 2, dtype=torch.int32), vert_ptr
        args = (self._stream(), b, h, w, bgr.data_ptr(), _native.ptr(anchors), path_ptr.data_ptr(), _native.ptr(path_closed),
                image_ptr.data_ptr(), q, int(margin), int(edge_cap), int(smooth), vert_ptr.data_ptr())
        if capacity > 0:
            verts = self.empty(int(capacity), 2, dtype=torch.int32)
            try:
                self.ctx.call("ggc_trace_paths", *args, verts.data_ptr(), int(capacity))
                return verts[:int(vert_ptr[-1].item())], vert_ptr
            except _native.GGCError:
                if int(vert_ptr[-1].item()) <= capacity:       # refused for another reason
                    raise
        else:
            self.ctx.call("ggc_trace_paths", *args, None, 0)
        n = int(vert_ptr[-1].item())
        verts = self.empty(n, 2, dtype=torch.int32)
        if n:
            self.ctx.call("ggc_trace_paths", *args, verts.data_ptr(), n)
        return verts, vert_ptr

    # ------------------------------------------------------------------ H5
    def wand_select(self, bgr, seeds, seed_ptr, tolerance=32, connectivity=8, sample=1, mask=None, select=True, counts=False):
        """Magic wand (ggc_wand_select, include/ggc.h H5): bgr (B,H,W,3) uint8, seeds (K,3) int32 = row, col, label and
        seed_ptr (B+1,) int32 on the device (upload_hints).  mask (B,H,W) uint8 GrabCut labels is painted in place;
        select=True gives the (B,H,W) uint8 selection, 255 | 0; counts=True the (B,2) int32 pixels decided by a
        foreground / background seed.  -> (mask, select, counts), None for what was not asked for.  A batch without a
        seed is a no-op of the entry: its selection and counts are the zeros they are made as."""
        b, h, w, _ = bgr.shape
        sel = torch.zeros(b, h, w, dtype=torch.uint8, device=self.device) if select else None
        cnt = torch.zeros(b, 2, dtype=torch.int32, device=self.device) if counts else None
        self.ctx.call("ggc_wand_select", self._stream(), b, h, w, bgr.data_ptr(), _native.ptr(seeds) or None, seed_ptr.data_ptr(),
                      int(tolerance), int(connectivity), int(sample), _native.ptr(mask), _native.ptr(sel), _native.ptr(cnt))
        return mask, sel, cnt

    def mask_outlines(self, masks, connectivity=8, capacity=None):
        """Mask outlines (ggc_mask_outlines, include/ggc.h K1): masks (B,H,W) uint8 on the device, any nonzero byte
        foreground -> (verts (V,2) int32 = row, col corners; loop_ptr (Q+1,); loop_info (Q,3) = area, outer, perimeter;
        image_ptr (B+1,); image_vert_ptr (B+1,)), all int32 on the device, verts and loop_ptr in ggc_apply_polygons'
        packing.  capacity None: one counting call, then one filling call of exactly the counted size.  capacity =
        (loops, vertices) is a guess: one call fills buffers of that size and is repeated only when the guess was too
        small (the two image arrays are written either way)."""
        b, h, w = masks.shape
        image_ptr = torch.zeros(b + 1, dtype=torch.int32, device=self.device)
        image_vert_ptr = torch.zeros(b + 1, dtype=torch.int32, device=self.device)
        if b == 0:
            return (self.empty(0, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32, device=self.device),
                    self.empty(0, 3, dtype=torch.int32), image_ptr, image_vert_ptr)
        args = (self._stream(), b, h, w, masks.data_ptr(), int(connectivity), image_ptr.data_ptr(), image_vert_ptr.data_ptr())

        def fill(q, v):
            loop_ptr = torch.zeros(q + 1, dtype=torch.int32, device=self.device)
            loop_info = self.empty(max(q, 1), 3, dtype=torch.int32)         # an empty tensor has no address: NULL means "count only"
            verts = self.empty(max(v, 1), 2, dtype=torch.int32)
            self.ctx.call("ggc_mask_outlines", *args, loop_ptr.data_ptr(), loop_info.data_ptr(), verts.data_ptr(), q, v)
            n_q, n_v = int(image_ptr[-1].item()), int(image_vert_ptr[-1].item())
            return verts[:n_v], loop_ptr[:n_q + 1], loop_info[:n_q], image_ptr, image_vert_ptr

        if capacity is not None:
            q, v = (max(int(c), 0) for c in capacity)
            try:
                return fill(q, v)
            except _native.GGCError:
                if int(image_ptr[-1].item()) <= q and int(image_vert_ptr[-1].item()) <= v:      # refused for another reason
                    raise
        else:
            self.ctx.call("ggc_mask_outlines", *args, None, None, None, 0, 0)
        return fill(int(image_ptr[-1].item()), int(image_vert_ptr[-1].item()))

    def mask_distance(self, masks, border_background=False, max_distance2=0, out=None) -> torch.Tensor:
        """The exact signed squared Euclidean distance transform (ggc_mask_distance, include/ggc.h K2): masks (B,H,W) uint8
        on the device, any nonzero byte foreground -> (B,H,W) int32: +d2 to the nearest foreground pixel on the background,
        -d2 to the nearest background pixel on the foreground, magnitude 2^31 - 1 where there is none or where it exceeds
        max_distance2 > 0.  border_background: everything outside the image is background.  No synchronisation."""
        b, h, w = masks.shape
        if out is None:
            out = self.empty(b, h, w, dtype=torch.int32)
        self.ctx.call("ggc_mask_distance", self._stream(), b, h, w, masks.data_ptr(), int(bool(border_background)),
                      int(max_distance2), out.data_ptr())
        return out

    def modify_mask(self, masks, op, r2_a, r2_b=0, border_background=False, out=None) -> torch.Tensor:
        """One modifier of ggc_modify_mask (include/ggc.h K3) on masks (B,H,W) uint8 on the device: op 0 grow, 1 shrink,
        2 border, 3 open, 4 close, 5 trimap; r2_a, r2_b squared radii.  -> (B,H,W) uint8 (0/1, the trimap 0/128/255); out
        may be masks itself.  No synchronisation."""
        b, h, w = masks.shape
        if out is None:
            out = torch.empty_like(masks)
        self.ctx.call("ggc_modify_mask", self._stream(), b, h, w, masks.data_ptr(), int(op), int(r2_a), int(r2_b),
                      int(bool(border_background)), out.data_ptr())
        return out

    def next_click(self, pred, gt) -> torch.Tensor:
        """The next simulated click of the NoC protocol per image (ggc_next_click): pred, gt (B,H,W) uint8, nonzero =
        foreground -> (B,4) int32 on the device = row, col, label (1 = fg, 0 = bg), d2; (-1,-1,-1,0) where pred == gt."""
        b, h, w = pred.shape
        if tuple(gt.shape) != (b, h, w):
            raise ValueError(f"next_click: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape")
        out = self.empty(b, 4, dtype=torch.int32)
        self.ctx.call("ggc_next_click", self._stream(), b, h, w, pred.data_ptr(), gt.data_ptr(), out.data_ptr())
        return out

    # ------------------------------------------------------------------ C0-C6, K0, O0, R0
    def grabcut(self, image, mask, n_iter=5, mode=0, rects=None, seed=0, bgd=None, fgd=None):
        """In place on mask; returns (binary, mask, bgd_model, fgd_model)."""
        b, h, w, _ = image.shape
        if bgd is None:
            bgd = torch.zeros(b, 65, dtype=torch.float64, device=self.device)
        if fgd is None:
            fgd = torch.zeros(b, 65, dtype=torch.float64, device=self.device)
        binary = self.empty(b, h, w, dtype=torch.uint8)
        r = None if rects is None else np.ascontiguousarray(rects, dtype=np.int32).reshape(b, 4)
        self.ctx.call("ggc_grabcut", self._stream(), b, h, w, image.data_ptr(), mask.data_ptr(),
                      None if r is None else r.ctypes.data, bgd.data_ptr(), fgd.data_ptr(), int(n_iter), int(mode),
                      int(seed), binary.data_ptr())
        return binary, mask, bgd, fgd

    def convert_color8(self, bgr: torch.Tensor, space: str) -> torch.Tensor:
        """(…,3) uint8 BGR -> 8-bit HSV / Lab in the style of cv2.cvtColor (ggc_convert_color8)."""
        out = torch.empty_like(bgr)
        self.ctx.call("ggc_convert_color8", self._stream(), int(bgr.numel() // 3), bgr.data_ptr(), {"hsv": 0, "lab": 1}[space],
                      out.data_ptr())
        return out

    def clean_mask(self, mask, min_area_ratio=0.002, keep_largest=False, out=None) -> torch.Tensor:
        b, h, w = mask.shape
        if out is None:
            out = torch.empty_like(mask)
        self.ctx.call("ggc_clean_mask", self._stream(), b, h, w, mask.data_ptr(), float(min_area_ratio),
                      int(bool(keep_largest)), out.data_ptr())
        return out

    def compose(self, bgr, binary, alpha=0.45, tint_bgr=(100, 220, 0), out=None):
        b, h, w, _ = bgr.shape
        overlay, rgba = out if out is not None else (self.empty(b, h, w, 3, dtype=torch.uint8), self.empty(b, h, w, 4, dtype=torch.uint8))
        self.ctx.call("ggc_compose_outputs", self._stream(), b, h, w, bgr.data_ptr(), binary.data_ptr(), float(alpha),
                      int(tint_bgr[0]), int(tint_bgr[1]), int(tint_bgr[2]), overlay.data_ptr(), rgba.data_ptr())
        return overlay, rgba

    def alpha_matte(self, bgr, binary, radius=4, eps=1e-4, want_rgba=False, out=None):
        """Soft alpha matte of binary (B,H,W) uint8 (nonzero = foreground) under bgr (B,H,W,3) uint8 (ggc_alpha_matte).
        -> alpha (B,H,W) float32 in [0,1], or (alpha, rgba (B,H,W,4) uint8) with want_rgba; out: the same, preallocated."""
        check_matte_args(radius, eps)
        b, h, w, _ = bgr.shape
        if tuple(binary.shape) != (b, h, w):
            raise ValueError(f"alpha_matte: binary {tuple(binary.shape)} does not match bgr {tuple(bgr.shape)}")
        if out is not None:
            alpha, rgba = out if want_rgba else (out, None)
        else:
            alpha = self.empty(b, h, w)
            rgba = self.empty(b, h, w, 4, dtype=torch.uint8) if want_rgba else None
        self.ctx.call("ggc_alpha_matte", self._stream(), b, h, w, bgr.data_ptr(), binary.data_ptr(), int(radius),
                      float(eps), alpha.data_ptr(), _native.ptr(rgba))
        return (alpha, rgba) if want_rgba else alpha

    def upsample_matte(self, bgr, binary, bgr_full, radius=4, eps=1e-4, want_alpha=True, want_binary=True,
                       want_rgba=False, out=None):
        """The soft matte of binary (B,H,W) uint8 under bgr (B,H,W,3) uint8, carried to bgr_full (B,H1,W1,3) uint8 with
        H1 >= H, W1 >= W by the fast guided filter (ggc_upsample_matte).  -> (alpha (B,H1,W1) float32, binary
        (B,H1,W1) uint8 = alpha >= 0.5, rgba (B,H1,W1,4) uint8), each None unless wanted; out: the same, preallocated."""
        check_matte_args(radius, eps)
        check_upsample_shapes(tuple(bgr.shape), tuple(binary.shape), tuple(bgr_full.shape), "upsample_matte")
        if not (want_alpha or want_binary or want_rgba):
            raise ValueError("upsample_matte: ask for at least one of alpha, binary and rgba")
        b, h, w, _ = bgr.shape
        h1, w1 = int(bgr_full.shape[1]), int(bgr_full.shape[2])
        if out is None:
            out = (self.empty(b, h1, w1) if want_alpha else None,
                   self.empty(b, h1, w1, dtype=torch.uint8) if want_binary else None,
                   self.empty(b, h1, w1, 4, dtype=torch.uint8) if want_rgba else None)
        alpha, mask, rgba = out
        self.ctx.call("ggc_upsample_matte", self._stream(), b, h, w, bgr.data_ptr(), binary.data_ptr(), h1, w1,
                      bgr_full.data_ptr(), int(radius), float(eps), _native.ptr(alpha), _native.ptr(mask),
                      _native.ptr(rgba))
        return alpha, mask, rgba

    def closed_form_matte(self, bgr, binary, radius, eps, band, max_iter, tol, want_rgba=False, out=None):
        """Closed-form alpha matte of binary (B,H,W) uint8 (nonzero = foreground) under bgr (B,H,W,3) uint8
        (ggc_closed_form_matte): the matting Laplacian solved on the band of `band` pixels around the mask's edge.
        -> (alpha (B,H,W) float32 in [0,1], iters (B,) int32, rel_residual (B,) float64), with want_rgba also rgba
        (B,H,W,4) uint8 after alpha; out: (alpha, rgba or None), preallocated.  The call synchronises its stream."""
        check_closed_form_args(radius, eps, band, max_iter, tol)
        b, h, w, _ = bgr.shape
        if tuple(binary.shape) != (b, h, w):
            raise ValueError(f"closed_form_matte: binary {tuple(binary.shape)} does not match bgr {tuple(bgr.shape)}")
        check_closed_form_shape(h, w, radius)
        if out is not None:
            alpha, rgba = out
        else:
            alpha = self.empty(b, h, w)
            rgba = self.empty(b, h, w, 4, dtype=torch.uint8) if want_rgba else None
        iters = self.empty(b, dtype=torch.int32)
        rel = self.empty(b, dtype=torch.float64)
        self.ctx.call("ggc_closed_form_matte", self._stream(), b, h, w, bgr.data_ptr(), binary.data_ptr(), int(radius),
                      float(eps), int(band), int(max_iter), float(tol), _native.ptr(alpha), _native.ptr(rgba), None,
                      iters.data_ptr(), rel.data_ptr())
        return (alpha, rgba, iters, rel) if want_rgba else (alpha, iters, rel)

    def trimap_matte(self, bgr, trimap, radius, eps, max_iter, tol, alpha0=None, want_rgba=False, out=None, warm=False):
        """Closed-form alpha matte of bgr (B,H,W,3) uint8 on the unknown region of trimap (B,H,W) uint8: 255 foreground,
        0 background, every other byte unknown (ggc_trimap_matte).  alpha0 (B,H,W) float32 or None: where the unknown
        pixels start (clamped to [0, 1]; 0.5 without it).  -> (alpha (B,H,W) float32 in [0,1], iters (B,) int32,
        rel_residual (B,) float64), with want_rgba also rgba (B,H,W,4) uint8 after alpha; out: (alpha, rgba or None),
        preallocated.  The call synchronises its stream.  warm=True (needs alpha0; ggc_trimap_matte_warm): an image
        stops on the residual of the 0.5 start instead of on its own start's, so a good alpha0 saves iterations, and
        rel_residual is relative to that."""
        check_closed_form_args(radius, eps, 0, max_iter, tol)
        if warm and alpha0 is None:
            raise ValueError("trimap_matte: warm=True needs alpha0, the start it is warm from")
        b, h, w, _ = bgr.shape
        if tuple(trimap.shape) != (b, h, w):
            raise ValueError(f"trimap_matte: trimap {tuple(trimap.shape)} does not match bgr {tuple(bgr.shape)}")
        if trimap.dtype != torch.uint8:
            raise ValueError(f"trimap_matte: trimap must be uint8, got {trimap.dtype}")
        if alpha0 is not None:
            if tuple(alpha0.shape) != (b, h, w):
                raise ValueError(f"trimap_matte: alpha0 {tuple(alpha0.shape)} does not match bgr {tuple(bgr.shape)}")
            if alpha0.dtype != torch.float32:
                raise ValueError(f"trimap_matte: alpha0 must be float32, got {alpha0.dtype}")
            alpha0 = alpha0.contiguous()
        check_closed_form_shape(h, w, radius)
        if out is not None:
            alpha, rgba = out
        else:
            alpha = self.empty(b, h, w)
            rgba = self.empty(b, h, w, 4, dtype=torch.uint8) if want_rgba else None
        iters = self.empty(b, dtype=torch.int32)
        rel = self.empty(b, dtype=torch.float64)
        trimap = trimap.contiguous()
        self.ctx.call("ggc_trimap_matte_warm" if warm else "ggc_trimap_matte", self._stream(), b, h, w, bgr.data_ptr(),
                      trimap.data_ptr(), int(radius),
                      float(eps), int(max_iter), float(tol), _native.ptr(alpha0), _native.ptr(alpha), _native.ptr(rgba),
                      None, iters.data_ptr(), rel.data_ptr())
        return (alpha, rgba, iters, rel) if want_rgba else (alpha, iters, rel)

    def lift_trimap(self, trimap, alpha, full_shape, grow=0, want_trimap=True, want_alpha0=True):
        """trimap (B,H,W) uint8 (255 foreground, 0 background, else unknown) and alpha (B,H,W) float32 carried to
        full_shape = (H1, W1) >= (H, W) (ggc_lift_trimap): the trimap and the start of a solve at that size.
        -> (trimap_full (B,H1,W1) uint8 with unknown = 128, dilated by grow pixels; alpha0_full (B,H1,W1) float32, the
        bilinear interpolation of the clamped alpha), each None unless wanted."""
        check_lift_args(tuple(trimap.shape), None if alpha is None else tuple(alpha.shape), full_shape, grow)
        if not (want_trimap or want_alpha0):
            raise ValueError("lift_trimap: ask for at least one of trimap and alpha0")
        if trimap.dtype != torch.uint8:
            raise ValueError(f"lift_trimap: trimap must be uint8, got {trimap.dtype}")
        if want_alpha0 and (alpha is None or alpha.dtype != torch.float32):
            raise ValueError(f"lift_trimap: alpha must be float32, got {None if alpha is None else alpha.dtype}")
        b, h, w = trimap.shape
        h1, w1 = int(full_shape[0]), int(full_shape[1])
        trimap = trimap.contiguous()
        alpha = alpha.contiguous() if want_alpha0 else None
        t_full = self.empty(b, h1, w1, dtype=torch.uint8) if want_trimap else None
        a_full = self.empty(b, h1, w1) if want_alpha0 else None
        self.ctx.call("ggc_lift_trimap", self._stream(), b, h, w, trimap.data_ptr(), _native.ptr(alpha), h1, w1, int(grow),
                      _native.ptr(t_full), _native.ptr(a_full))
        return t_full, a_full

    def closed_form_band(self, binary, band):
        """The unknown band closed_form_matte(binary, band) solves on, as a trimap (B,H,W) uint8: 128 on the band, else
        255 (binary != 0) (ggc_closed_form_band, the kernels of that solver's front end)."""
        check_closed_form_args(1, 1e-5, band, 1, 0.5)          # only the band is this entry's
        if binary.dim() != 3 or binary.dtype != torch.uint8:
            raise ValueError(f"closed_form_band: binary must be (B,H,W) uint8, got {tuple(binary.shape)} {binary.dtype}")
        b, h, w = binary.shape
        binary = binary.contiguous()
        trimap = self.empty(b, h, w, dtype=torch.uint8)
        self.ctx.call("ggc_closed_form_band", self._stream(), b, h, w, binary.data_ptr(), int(band), trimap.data_ptr())
        return trimap

    def lift_labels(self, binary, full_shape, band, want_labels=True, want_mask=False):
        """binary (B,H,W) uint8 (nonzero = foreground) carried to full_shape = (H1, W1) >= (H, W) as the start of a banded
        cut there (ggc_lift_labels).  -> (labels (B,H1,W1) uint8: GrabCut labels, probable (2, 3) within band pixels of
        the lifted mask's edge and definite (0, 1) elsewhere; mask_full (B,H1,W1) uint8 {0, 1}: the lifted mask, the
        bilinear interpolation >= 0.5), each None unless wanted."""
        check_full_cut_args(tuple(binary.shape), full_shape, band)
        if not (want_labels or want_mask):
            raise ValueError("lift_labels: ask for at least one of labels and mask")
        if binary.dtype != torch.uint8:
            raise ValueError(f"lift_labels: binary must be uint8, got {binary.dtype}")
        b, h, w = binary.shape
        h1, w1 = int(full_shape[0]), int(full_shape[1])
        binary = binary.contiguous()
        labels = self.empty(b, h1, w1, dtype=torch.uint8) if want_labels else None
        mask = self.empty(b, h1, w1, dtype=torch.uint8) if want_mask else None
        self.ctx.call("ggc_lift_labels", self._stream(), b, h, w, binary.data_ptr(), h1, w1, int(band), _native.ptr(labels),
                      _native.ptr(mask))
        return labels, mask

    def cut_mask_full(self, binary, bgr_full, band, n_iter=1, seed=0, color_space="rgb", min_area_ratio=0.002,
                      keep_largest=False, out=None, max_pixels=None, want_labels=False):
        """The banded cut of cut_mask_full on a batch: binary (B,H,W) uint8 and bgr_full (B,H1,W1,3) uint8 -> (B,H1,W1)
        uint8 {0, 1} (out: the same, preallocated).  ggc_lift_labels, ggc_convert_color8 (color_space other than rgb),
        ggc_grabcut(mode 0, n_iter) cold from the labels with image b on seed + b, ggc_clean_mask.  max_pixels: the
        images go through those entries in sub-batches of at most that many pixels (at least one image); every entry
        is independent per image, so the split does not change the result."""
        b, h1, w1, _ = bgr_full.shape
        if out is None:
            out = self.empty(b, h1, w1, dtype=torch.uint8)
        step = b if not max_pixels else max(1, int(max_pixels) // (h1 * w1))
        kept = []
        for lo in range(0, b, max(step, 1)):
            hi = min(b, lo + step)
            labels, _ = self.lift_labels(binary[lo:hi], (h1, w1), band)
            if want_labels:
                kept.append(labels.clone())
            img = bgr_full[lo:hi] if color_space == "rgb" else self.convert_color8(bgr_full[lo:hi].contiguous(), color_space)
            cut = self.grabcut(img, labels, n_iter, 0, None, seed + lo)[0]
            self.clean_mask(cut, min_area_ratio, keep_largest, out=out[lo:hi])
        return (out, torch.cat(kept)) if want_labels else out

    def closed_form_full(self, bgr, trimap, alpha, bgr_full, radius, eps, grow, max_iter, tol, out=None):
        """The full-resolution end of closed_form_matte_full / trimap_matte_full: a working-size trimap (B,H,W) uint8 and
        its solved alpha (B,H,W) float32 lifted to bgr_full (B,H1,W1,3) uint8 (lift_trimap), then the warm solve there.
        -> (alpha_full (B,H1,W1) float32, rgba_full (B,H1,W1,4) uint8, iters (B,), rel_residual (B,)); out: (alpha_full,
        rgba_full), preallocated."""
        t_full, a0_full = self.lift_trimap(trimap, alpha, tuple(bgr_full.shape[1:3]), grow)
        return self.trimap_matte(bgr_full, t_full, radius, eps, max_iter, tol, alpha0=a0_full, want_rgba=True, out=out,
                                 warm=True)

    def estimate_foreground(self, bgr, alpha, eps_r, omega, max_iter, tol, want_rgba=False, out=None):
        """Foreground colours of bgr (B,H,W,3) uint8 under alpha (B,H,W) float32 (ggc_estimate_foreground): F where
        alpha is fractional, the image's bytes elsewhere.
        -> (foreground (B,H,W,3) uint8, iters (B,) int32, rel_residual (B,) float64), with want_rgba also rgba
        (B,H,W,4) uint8, that colour with round(255 alpha), after foreground; out: (foreground, rgba or None),
        preallocated.  The call synchronises its stream."""
        check_foreground_args(eps_r, omega, max_iter, tol)
        b, h, w, _ = bgr.shape
        if tuple(alpha.shape) != (b, h, w):
            raise ValueError(f"estimate_foreground: alpha {tuple(alpha.shape)} does not match bgr {tuple(bgr.shape)}")
        if alpha.dtype != torch.float32:
            raise ValueError(f"estimate_foreground: alpha must be float32, got {alpha.dtype}")
        if h > UPSAMPLE_SIDE_MAX or w > UPSAMPLE_SIDE_MAX:
            raise ValueError(f"estimate_foreground takes images of at most {UPSAMPLE_SIDE_MAX} on a side, got {h}x{w}")
        if out is not None:
            fg, rgba = out
        else:
            fg = self.empty(b, h, w, 3, dtype=torch.uint8)
            rgba = self.empty(b, h, w, 4, dtype=torch.uint8) if want_rgba else None
        iters = self.empty(b, dtype=torch.int32)
        rel = self.empty(b, dtype=torch.float64)
        self.ctx.call("ggc_estimate_foreground", self._stream(), b, h, w, bgr.data_ptr(), alpha.data_ptr(), float(eps_r),
                      float(omega), int(max_iter), float(tol), _native.ptr(fg), _native.ptr(rgba), None, None,
                      iters.data_ptr(), rel.data_ptr())
        return (fg, rgba, iters, rel) if want_rgba else (fg, iters, rel)

    def composite_over(self, rgba, background, offsets, out=None):
        """The BGRA cut-outs rgba (B,Hs,Ws,4) uint8 placed on background (B,H,W,3) uint8 (ggc_composite_over): integer
        alpha-over, (a c + (255 - a) bg + 127) // 255.  offsets: (B,2) integers on the host, row and column of each
        cut-out's pixel (0, 0) in its background, negative allowed.
        -> (B,H,W,3) uint8; out: preallocated (it may be background).  The call does not synchronise."""
        off = check_composite_args(tuple(rgba.shape), tuple(background.shape), offsets, (rgba.dtype, background.dtype), 4,
                                   "composite_over")
        b, hs, ws, _ = rgba.shape
        _, h, w, _ = background.shape
        if out is None:
            out = self.empty(b, h, w, 3, dtype=torch.uint8)
        elif tuple(out.shape) != (b, h, w, 3) or out.dtype != torch.uint8:
            raise ValueError(f"composite_over: out must be {(b, h, w, 3)} uint8, got {tuple(out.shape)} {out.dtype}")
        rgba, background = rgba.contiguous(), background.contiguous()
        self.ctx.call("ggc_composite_over", self._stream(), b, hs, ws, rgba.data_ptr(), h, w, background.data_ptr(),
                      self.to_device(off).data_ptr(), out.data_ptr())
        return out

    def poisson_clone(self, source, mask, target, offsets, mixed, max_iter, tol, want_raw=False):
        """Seamless cloning (ggc_poisson_clone): the pixels of source (B,Hs,Ws,3) uint8 selected by mask (B,Hs,Ws) uint8
        (non-zero) cloned into target (B,H,W,3) uint8 in the gradient domain, with the source's gradients (mixed False)
        or the stronger of the source's and the target's (mixed True).  offsets: (B,2) integers on the host, as
        composite_over's, each within +-32768.
        -> (composite (B,H,W,3) uint8, n_omega (B,) int32, iters (B,) int32, rel_residual (B,) float64), with want_raw
        also raw (B,H,W,3) float64, the unclamped solution, after composite.  The call synchronises its stream."""
        off = check_composite_args(tuple(source.shape), tuple(target.shape), offsets, (source.dtype, target.dtype), 3,
                                   "poisson_clone")
        check_clone_args(mixed, max_iter, tol)
        b, hs, ws, _ = source.shape
        _, h, w, _ = target.shape
        if tuple(mask.shape) != (b, hs, ws):
            raise ValueError(f"poisson_clone: mask {tuple(mask.shape)} does not match source {tuple(source.shape)}")
        if mask.dtype != torch.uint8:
            raise ValueError(f"poisson_clone: mask must be uint8, got {mask.dtype}")
        comp = self.empty(b, h, w, 3, dtype=torch.uint8)
        raw = self.empty(b, h, w, 3, dtype=torch.float64) if want_raw else None
        n_omega, iters = self.empty(b, dtype=torch.int32), self.empty(b, dtype=torch.int32)
        rel = self.empty(b, dtype=torch.float64)
        source, mask, target = source.contiguous(), mask.contiguous(), target.contiguous()
        self.ctx.call("ggc_poisson_clone", self._stream(), b, hs, ws, source.data_ptr(), mask.data_ptr(), h, w,
                      target.data_ptr(), self.to_device(off).data_ptr(), int(bool(mixed)), int(max_iter), float(tol),
                      comp.data_ptr(), _native.ptr(raw), n_omega.data_ptr(), iters.data_ptr(), rel.data_ptr())
        return (comp, raw, n_omega, iters, rel) if want_raw else (comp, n_omega, iters, rel)

    def matte_errors(self, pred_u8, gt_u8, region=None, want_grad=True, want_levels=False):
        """The four matte errors of pred_u8 against gt_u8, both (B,H,W) uint8 alpha levels on the device
        (ggc_matte_errors); region (B,H,W) uint8 or None restricts the sums to its nonzero pixels.
        -> (sums (B,4) int64 = n, SAD, SSE, CONN, grad (B,) float64 or None, levels (B,H,W) uint8 or None), on the
        device.  The call does not synchronise."""
        check_matte_eval_args(tuple(pred_u8.shape), tuple(gt_u8.shape), None if region is None else tuple(region.shape),
                              (pred_u8.dtype, gt_u8.dtype) + (() if region is None else (region.dtype,)))
        b, h, w = pred_u8.shape
        sums = self.empty(b, 4, dtype=torch.int64)
        grad = self.empty(b, dtype=torch.float64) if want_grad else None
        levels = self.empty(b, h, w, dtype=torch.uint8) if want_levels else None
        pred_u8, gt_u8 = pred_u8.contiguous(), gt_u8.contiguous()
        region = None if region is None else region.contiguous()
        self.ctx.call("ggc_matte_errors", self._stream(), b, h, w, pred_u8.data_ptr(), gt_u8.data_ptr(),
                      _native.ptr(region), sums.data_ptr(), _native.ptr(grad), _native.ptr(levels))
        return sums, grad, levels

    def iou(self, pred, gt):
        """-> (iou (B,) float64, counts (B,3) int64 = tp, fp, fn), on device."""
        b, h, w = pred.shape
        iou = self.empty(b, dtype=torch.float64)
        cnt = self.empty(b, 3, dtype=torch.int64)
        self.ctx.call("ggc_mask_iou", self._stream(), b, h, w, pred.data_ptr(), gt.data_ptr(), iou.data_ptr(),
                      cnt.data_ptr())
        return iou, cnt


MATTE_RADIUS_MAX = 64
MATTE_EPS_MIN = 1e-12


def check_matte_args(radius, eps) -> None:
    """The argument range of ggc_alpha_matte, checked on the host so that a bad value is a ValueError."""
    if int(radius) != radius or not 1 <= int(radius) <= MATTE_RADIUS_MAX:
        raise ValueError(f"matte radius must be an integer in 1..{MATTE_RADIUS_MAX}, got {radius}")
    if not (np.isfinite(eps) and float(eps) >= MATTE_EPS_MIN):
        raise ValueError(f"matte eps must be finite and >= {MATTE_EPS_MIN:g}, got {eps}")


CF_RADIUS_MAX = 8
CF_BAND_MAX = 64
CF_MAX_ITER_MAX = 100000


def check_closed_form_args(radius, eps, band, max_iter, tol) -> None:
    """The argument range of ggc_closed_form_matte, checked on the host so that a bad value is a ValueError."""
    if int(radius) != radius or not 1 <= int(radius) <= CF_RADIUS_MAX:
        raise ValueError(f"closed-form radius must be an integer in 1..{CF_RADIUS_MAX}, got {radius}")
    if not (np.isfinite(eps) and 1e-12 <= float(eps) <= 1.0):
        raise ValueError(f"closed-form eps must be in [1e-12, 1], got {eps}")
    if int(band) != band or not 0 <= int(band) <= CF_BAND_MAX:
        raise ValueError(f"closed-form band must be an integer in 0..{CF_BAND_MAX}, got {band}")
    if int(max_iter) != max_iter or not 1 <= int(max_iter) <= CF_MAX_ITER_MAX:
        raise ValueError(f"closed-form max_iter must be an integer in 1..{CF_MAX_ITER_MAX}, got {max_iter}")
    if not (np.isfinite(tol) and 1e-12 <= float(tol) < 1.0):
        raise ValueError(f"closed-form tol must be in [1e-12, 1), got {tol}")


def check_closed_form_shape(h, w, radius) -> None:
    """Every window of the closed-form matte lies inside the image: H, W >= 2 radius + 1."""
    if h < 2 * int(radius) + 1 or w < 2 * int(radius) + 1:
        raise ValueError(f"closed-form matte needs H, W >= 2r+1 = {2 * int(radius) + 1}, got {h}x{w}")
    if h > UPSAMPLE_SIDE_MAX or w > UPSAMPLE_SIDE_MAX:
        raise ValueError(f"closed-form matte takes images of at most {UPSAMPLE_SIDE_MAX} on a side, got {h}x{w}")


LIFT_GROW_MAX = 64


def check_lift_args(trimap_shape, alpha_shape, full_shape, grow) -> None:
    """The rules of ggc_lift_trimap, checked on the host so that a bad argument is a ValueError: trimap and alpha
    (B,H,W), full_shape (H1, W1) with H <= H1 <= 32768 and W <= W1 <= 32768, grow an integer in 0..64."""
    if len(trimap_shape) != 3 or min(trimap_shape[1:]) < 1:
        raise ValueError(f"lift_trimap: trimap must be (B,H,W), got {tuple(trimap_shape)}")
    if alpha_shape is not None and tuple(alpha_shape) != tuple(trimap_shape):
        raise ValueError(f"lift_trimap: alpha {tuple(alpha_shape)} does not match trimap {tuple(trimap_shape)}")
    if len(full_shape) != 2:
        raise ValueError(f"lift_trimap: full_shape must be (H1, W1), got {tuple(full_shape)}")
    h, w = trimap_shape[1:]
    if not (h <= full_shape[0] <= UPSAMPLE_SIDE_MAX and w <= full_shape[1] <= UPSAMPLE_SIDE_MAX):
        raise ValueError(f"lift_trimap: full size {tuple(full_shape)} must be at least the working size {(h, w)} and at "
                         f"most {UPSAMPLE_SIDE_MAX} on a side")
    if isinstance(grow, bool) or int(grow) != grow or not 0 <= int(grow) <= LIFT_GROW_MAX:
        raise ValueError(f"lift_trimap: grow must be an integer in 0..{LIFT_GROW_MAX}, got {grow}")


FULL_CUT_BAND_MAX = 64
FULL_CUT_ITER_MAX = 100
FULL_CUT_PIXEL_MAX = 2 ** 28          # ggc_grabcut's limit on the pixels of one image


def default_full_cut_band(shape, full_shape) -> int:
    """The band of the full-resolution cut when none is given: one and a half working pixels,
    min(64, max(1, ceil(1.5 max(H1 / H, W1 / W)))) (a choice backed by DESIGN.md §5.18's table, not a tuned result)."""
    import math
    ratio = max(int(full_shape[0]) / int(shape[0]), int(full_shape[1]) / int(shape[1]))
    return min(FULL_CUT_BAND_MAX, max(1, math.ceil(1.5 * ratio)))


def check_full_cut_args(mask_shape, full_shape, band, n_iter=1, color_space="rgb") -> None:
    """The rules of ggc_lift_labels and of the cut after it, checked on the host so that a bad argument is a ValueError:
    mask (B,H,W), full_shape (H1, W1) with H <= H1 <= 32768, W <= W1 <= 32768 and H1 W1 < 2^28, band an integer in 0..64,
    n_iter an integer in 1..100, color_space rgb | hsv | lab."""
    if len(mask_shape) != 3 or min(mask_shape[1:]) < 1:
        raise ValueError(f"full cut: mask must be (B,H,W), got {tuple(mask_shape)}")
    if len(full_shape) != 2:
        raise ValueError(f"full cut: full_shape must be (H1, W1), got {tuple(full_shape)}")
    h, w = mask_shape[1:]
    if not (h <= full_shape[0] <= UPSAMPLE_SIDE_MAX and w <= full_shape[1] <= UPSAMPLE_SIDE_MAX):
        raise ValueError(f"full cut: full size {tuple(full_shape)} must be at least the working size {(h, w)} and at "
                         f"most {UPSAMPLE_SIDE_MAX} on a side")
    if int(full_shape[0]) * int(full_shape[1]) >= FULL_CUT_PIXEL_MAX:
        raise ValueError(f"full cut: GrabCut takes images below 2^28 pixels, got {tuple(full_shape)}")
    if isinstance(band, bool) or int(band) != band or not 0 <= int(band) <= FULL_CUT_BAND_MAX:
        raise ValueError(f"full cut: band must be an integer in 0..{FULL_CUT_BAND_MAX}, got {band}")
    if isinstance(n_iter, bool) or int(n_iter) != n_iter or not 1 <= int(n_iter) <= FULL_CUT_ITER_MAX:
        raise ValueError(f"full cut: n_iter must be an integer in 1..{FULL_CUT_ITER_MAX}, got {n_iter}")
    if str(color_space).lower() not in ("rgb", "hsv", "lab"):
        raise ValueError(f"unknown color_space '{color_space}': rgb | hsv | lab")


FG_OMEGA_MAX = 1e3


def check_foreground_args(eps_r, omega, max_iter, tol) -> None:
    """The argument range of ggc_estimate_foreground, checked on the host so that a bad value is a ValueError."""
    if not (np.isfinite(eps_r) and 0.0 <= float(eps_r) <= 1.0):
        raise ValueError(f"foreground eps_r must be in [0, 1], got {eps_r}")
    if not (np.isfinite(omega) and 0.0 <= float(omega) <= FG_OMEGA_MAX):
        raise ValueError(f"foreground omega must be in [0, {FG_OMEGA_MAX:g}], got {omega}")
    if not np.float32(eps_r) + np.float32(omega) > 0.0:
        raise ValueError("foreground eps_r + omega must be positive (as float32)")
    if int(max_iter) != max_iter or not 1 <= int(max_iter) <= CF_MAX_ITER_MAX:
        raise ValueError(f"foreground max_iter must be an integer in 1..{CF_MAX_ITER_MAX}, got {max_iter}")
    if not (np.isfinite(tol) and 1e-12 <= float(tol) < 1.0):
        raise ValueError(f"foreground tol must be in [1e-12, 1), got {tol}")


CLONE_OFFSET_MAX = 32768
CLONE_BATCH_MAX = 65535


def check_composite_args(source_shape, target_shape, offsets, dtypes=(), channels=4, what="composite_over") -> np.ndarray:
    """The shape rules of ggc_composite_over and ggc_poisson_clone, checked on the host so that a bad argument is a
    ValueError: source (B,Hs,Ws,channels) and target (B,H,W,3) uint8 with B <= 65535 and every side in 1..32768; offsets
    (B,2) integers within +-32768.  -> the offsets as a contiguous (B,2) int32 array."""
    if len(source_shape) != 4 or source_shape[3] != channels or min(source_shape[1:3]) < 1:
        raise ValueError(f"{what}: the source must be (B,Hs,Ws,{channels}), got {tuple(source_shape)}")
    if len(target_shape) != 4 or target_shape[3] != 3 or min(target_shape[1:3]) < 1:
        raise ValueError(f"{what}: the background must be (B,H,W,3), got {tuple(target_shape)}")
    if source_shape[0] != target_shape[0]:
        raise ValueError(f"{what}: {source_shape[0]} sources for {target_shape[0]} backgrounds")
    if source_shape[0] > CLONE_BATCH_MAX or max(*source_shape[1:3], *target_shape[1:3]) > UPSAMPLE_SIDE_MAX:
        raise ValueError(f"{what} takes at most {CLONE_BATCH_MAX} images of at most {UPSAMPLE_SIDE_MAX} on a side, got "
                         f"{tuple(source_shape)} on {tuple(target_shape)}")
    for d in dtypes:
        if str(d).replace("torch.", "") != "uint8":                  # a torch or a numpy dtype
            raise ValueError(f"{what}: images must be uint8, got {d}")
    off = np.asarray(offsets)
    if off.dtype.kind not in "iu" or off.shape != (source_shape[0], 2):
        raise ValueError(f"{what}: offsets must be ({source_shape[0]}, 2) integers (row, col), got {off.shape} {off.dtype}")
    if off.size and np.abs(off.astype(np.int64)).max() > CLONE_OFFSET_MAX:
        raise ValueError(f"{what}: offsets must lie within +-{CLONE_OFFSET_MAX}, got {off.tolist()}")
    return np.ascontiguousarray(off, np.int32)


def check_clone_args(mixed, max_iter, tol) -> None:
    """The argument range of ggc_poisson_clone, checked on the host so that a bad value is a ValueError."""
    if not isinstance(mixed, (bool, np.bool_)) and mixed not in (0, 1):
        raise ValueError(f"clone mixed must be a bool, got {mixed!r}")
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or not 1 <= int(max_iter) <= CF_MAX_ITER_MAX:
        raise ValueError(f"clone max_iter must be an integer in 1..{CF_MAX_ITER_MAX}, got {max_iter}")
    if not (np.isfinite(tol) and 1e-12 <= float(tol) < 1.0):
        raise ValueError(f"clone tol must be in [1e-12, 1), got {tol}")


MATTE_EVAL_BATCH_MAX = 65535


def check_matte_eval_args(pred_shape, gt_shape, region_shape=None, dtypes=()) -> None:
    """The shape rules of ggc_matte_errors, checked on the host so that a bad argument is a ValueError: pred, gt and
    region (B,H,W) uint8 of one shape, B <= 65535, H, W in 1..32768, H W < 2^31."""
    if len(pred_shape) != 3:
        raise ValueError(f"matte_errors: mattes must be (B,H,W), got {tuple(pred_shape)}")
    if tuple(gt_shape) != tuple(pred_shape):
        raise ValueError(f"matte_errors: pred {tuple(pred_shape)} and gt {tuple(gt_shape)} differ in shape")
    if region_shape is not None and tuple(region_shape) != tuple(pred_shape):
        raise ValueError(f"matte_errors: region {tuple(region_shape)} does not match the mattes {tuple(pred_shape)}")
    b, h, w = (int(v) for v in pred_shape)
    if b > MATTE_EVAL_BATCH_MAX or not (1 <= h <= UPSAMPLE_SIDE_MAX and 1 <= w <= UPSAMPLE_SIDE_MAX) or h * w >= 2 ** 31:
        raise ValueError(f"matte_errors: B <= {MATTE_EVAL_BATCH_MAX}, H and W in 1..{UPSAMPLE_SIDE_MAX} and H*W < 2^31, "
                         f"got {tuple(pred_shape)}")
    for dt in dtypes:
        if dt != torch.uint8:
            raise ValueError(f"matte_errors: mattes and region must be uint8 levels, got {dt}")


UPSAMPLE_SIDE_MAX = 32768


def check_upsample_shapes(bgr_shape, mask_shape, full_shape, what="upsample") -> None:
    """The shape rules of ggc_upsample_matte, checked on the host so that a bad shape is a ValueError: bgr (B,H,W,3),
    mask (B,H,W), full (B,H1,W1,3) with H <= H1 <= 32768 and W <= W1 <= 32768."""
    if len(bgr_shape) != 4 or bgr_shape[3] != 3 or min(bgr_shape[:3]) < 1:
        raise ValueError(f"{what}: image must be (B,H,W,3), got {bgr_shape}")
    if tuple(mask_shape) != tuple(bgr_shape[:3]):
        raise ValueError(f"{what}: mask {tuple(mask_shape)} does not match image {tuple(bgr_shape)}")
    if len(full_shape) != 4 or full_shape[3] != 3 or full_shape[0] != bgr_shape[0]:
        raise ValueError(f"{what}: full image must be ({bgr_shape[0]},H1,W1,3), got {tuple(full_shape)}")
    if not (bgr_shape[1] <= full_shape[1] <= UPSAMPLE_SIDE_MAX and bgr_shape[2] <= full_shape[2] <= UPSAMPLE_SIDE_MAX):
        raise ValueError(f"{what}: full image {tuple(full_shape[1:3])} must be at least the working size "
                         f"{tuple(bgr_shape[1:3])} and at most {UPSAMPLE_SIDE_MAX} on a side")


def merge_graphs(parts: Sequence[DeviceGraphs], segments: torch.Tensor) -> DeviceGraphs:
    """The graphs of consecutive chunks of a batch as ONE packed batch (what build_graphs returns for the whole batch):
    node-indexed arrays are concatenated, edge endpoints shifted by the nodes that precede their chunk."""
    if len(parts) == 1:
        return parts[0]
    node_ptr, edge_ptr, src, dst = [np.zeros(1, np.int64)], [np.zeros(1, np.int64)], [], []
    n0 = e0 = 0
    for g in parts:
        node_ptr.append(g.node_ptr_host[1:] + n0)
        edge_ptr.append(g.edge_ptr_host[1:] + e0)
        src.append(g.edge_src + n0 if n0 else g.edge_src)
        dst.append(g.edge_dst + n0 if n0 else g.edge_dst)
        n0 += int(g.node_ptr_host[-1])
        e0 += int(g.edge_ptr_host[-1])
    node_ptr, edge_ptr = np.concatenate(node_ptr), np.concatenate(edge_ptr)
    dev = segments.device
    return DeviceGraphs(segments, torch.cat([g.n_nodes for g in parts]), node_ptr, edge_ptr,
                        torch.from_numpy(node_ptr.astype(np.int32)).to(dev, non_blocking=True),
                        torch.cat([g.x for g in parts]), torch.cat([g.centroids for g in parts]),
                        torch.cat([g.area_ratio for g in parts]), torch.cat(src), torch.cat(dst),
                        torch.cat([g.edge_attr for g in parts]))


_engines: dict[int, Engine] = {}


def get_engine(device="cuda") -> Engine:
    """Engine for a device spec ("cuda", "cuda:1", torch.device, int)."""
    if isinstance(device, int):
        idx = device
    else:
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"device '{device}': gcn_grabcut runs on MI355X (device 'cuda') only; "
                               "there is no CPU fallback")
        idx = dev.index if dev.index is not None else (torch.cuda.current_device() if torch.cuda.is_available() else 0)
    eng = _engines.get(idx)
    if eng is None:
        eng = Engine(idx)
        _engines[idx] = eng
    return eng
