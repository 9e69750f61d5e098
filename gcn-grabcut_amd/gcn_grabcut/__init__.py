"""
GCN-GrabCut on MI355X — host mirror of the reference package src/gcn_grabcut.

Same public names as the reference (__init__.py:57-81) for the per-image
segmentation hot path; all arithmetic runs in libggc_hip.so (hand-written
gfx950 kernels behind the C ABI of include/ggc.h).  `dataset` holds the
graph-cache writer behind tools/prepare_graphs.py; `losses`
and `trainer` train ResGCNNet on the MI355X (train.py); plotting stays out of scope.
"""
from ._constants import N_NODE_FEATS, N_EDGE_FEATS, N_PRIOR_FEATS, N_IMAGE_FEATS
from .data import Data, Batch
from .grabcut import GrabCut, GrabCutConfig, Label
from .graph_builder import (
    GraphBuilder, SuperpixelGraph, SuperpixelGraphConfig, compute_auto_prior, encode_user_hints, pack_hints,
    encode_geodesic_hints, pack_strokes, pack_polygons, pack_paths,
)
from .metrics import (
    evaluate, evaluate_batch, evaluate_trimap, boundary_f1, noc_summary, SegmentationMetrics, TrimapMetrics,
    evaluate_matte, evaluate_matte_batch, MatteMetrics,
)
from .model import (
    ResGCNNet, GCNTrimapNet, GATTrimapNet, build_model, _probs_to_trimap, probs_to_node_trimap, project_to_pixels,
    TRIMAP_BG, TRIMAP_FG, TRIMAP_PROB_BG, TRIMAP_PROB_FG, CLASS_BG, CLASS_UNK, CLASS_FG,
)
from .pipeline import (GCNGrabCutPipeline, ClosedFormMatte, ForegroundColours, FullResolution, SegmentationResult,
                       alpha_matte, clean_mask, closed_form_matte, estimate_foreground, guided_filter, refine_trimap,
                       closed_form_matte_full, lift_trimap, trimap_matte, trimap_matte_full,
                       trimap_matte_warm, upsample_mask, FullCut, cut_mask_full, lift_labels,
                       GeodesicHints, geodesic_hints, paint_strokes, stroke_pixels, paint_polygons, polygon_mask,
                       Scissors, trace_boundary, Wand, wand_select, wand_select_batch, paint_wand,
                       Outline, mask_outlines, mask_outlines_batch, outlines_svg_path, outlines_to_lassos,
                       ModifyMask, mask_distance, mask_distance_batch, modify_mask, modify_mask_batch, grow_mask,
                       shrink_mask, open_mask, close_mask, border_mask, mask_to_trimap,
                       Clone, composite_over, composite_over_batch, seamless_clone, seamless_clone_batch)
from .synthetic import synthetic_image, synthetic_batch
from .losses import FocalLoss, LabelSmoothingCE, TrimapLoss
from .trainer import Trainer, TrainConfig

__version__ = "0.3.0+mi355x.1"

__all__ = [
    "GrabCut", "GrabCutConfig", "Label",
    "GraphBuilder", "SuperpixelGraph", "SuperpixelGraphConfig", "compute_auto_prior", "encode_user_hints", "pack_hints",
    "N_NODE_FEATS", "N_EDGE_FEATS", "N_PRIOR_FEATS",
    "evaluate", "evaluate_batch", "evaluate_trimap", "boundary_f1", "noc_summary", "SegmentationMetrics", "TrimapMetrics",
    "evaluate_matte", "evaluate_matte_batch", "MatteMetrics",
    "GCNGrabCutPipeline", "FullResolution", "SegmentationResult", "alpha_matte", "clean_mask", "guided_filter",
    "refine_trimap", "upsample_mask", "ClosedFormMatte", "closed_form_matte", "ForegroundColours", "estimate_foreground",
    "trimap_matte", "trimap_matte_warm", "lift_trimap", "closed_form_matte_full", "trimap_matte_full",
    "FullCut", "cut_mask_full", "lift_labels",
    "GeodesicHints", "geodesic_hints", "encode_geodesic_hints",
    "pack_strokes", "paint_strokes", "stroke_pixels",
    "pack_polygons", "paint_polygons", "polygon_mask",
    "pack_paths", "Scissors", "trace_boundary",
    "Wand", "wand_select", "wand_select_batch", "paint_wand",
    "Outline", "mask_outlines", "mask_outlines_batch", "outlines_svg_path", "outlines_to_lassos",
    "ModifyMask", "mask_distance", "mask_distance_batch", "modify_mask", "modify_mask_batch", "grow_mask", "shrink_mask",
    "open_mask", "close_mask", "border_mask", "mask_to_trimap",
    "Clone", "composite_over", "composite_over_batch", "seamless_clone", "seamless_clone_batch",
    "ResGCNNet", "GCNTrimapNet", "GATTrimapNet", "build_model", "probs_to_node_trimap", "project_to_pixels",
    "Data", "Batch", "synthetic_image", "synthetic_batch",
    "FocalLoss", "LabelSmoothingCE", "TrimapLoss", "Trainer", "TrainConfig",
]
