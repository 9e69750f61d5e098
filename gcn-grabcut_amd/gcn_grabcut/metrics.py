"""
Segmentation metrics — host mirror of reference src/gcn_grabcut/metrics.py: `evaluate`
(:58-102), `boundary_f1` (:105-129), `evaluate_trimap` (:152-201), `evaluate_batch`
(:204-229).  Every metric is a ratio of integer tallies; the tallies (confusion counts,
eroded-boundary overlaps, trimap confusion) come from `ggc_eval_counts` on the MI355X,
the ratios use the reference's formulas (+1e-8 denominators) on the host.

Additive: `evaluate_matte` scores an alpha matte against the true one by the four errors of Rhemann et al. (CVPR 2009),
SAD, MSE, gradient and connectivity; the sums come from `ggc_matte_errors`, the conventional scaling is done here.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class SegmentationMetrics:
    iou: float
    dice: float
    precision: float
    recall: float
    f1: float
    pixel_accuracy: float
    boundary_f1: float = 0.0

    def __str__(self) -> str:
        return (f"IoU={self.iou:.4f}  Dice={self.dice:.4f}  Prec={self.precision:.4f}  Rec={self.recall:.4f}  "
                f"F1={self.f1:.4f}  PixAcc={self.pixel_accuracy:.4f}  BF1={self.boundary_f1:.4f}")

    def as_dict(self) -> dict:
        return {k: round(getattr(self, k), 4) for k in
                ("iou", "dice", "precision", "recall", "f1", "pixel_accuracy", "boundary_f1")}


def _counts(pred: np.ndarray, gt: np.ndarray, trimap=None, boundary_width: int = 0, device="cuda",
            binarize: bool = True) -> np.ndarray:
    """int64 [B,14] tallies of ggc_eval_counts for (B,H,W) or (H,W) inputs; binarize: masks as `!= 0` (astype(bool))."""
    import torch
    from ._engine import get_engine
    pred, gt = np.asarray(pred), np.asarray(gt)
    if pred.shape != gt.shape:
        raise ValueError(f"shape mismatch {pred.shape} vs {gt.shape}")
    if pred.ndim == 2:
        pred, gt = pred[None], gt[None]
        trimap = None if trimap is None else np.asarray(trimap)[None]
    eng = get_engine(device)
    b, h, w = pred.shape
    if binarize:
        pred, gt = pred != 0, gt != 0
    p = eng.to_device(np.ascontiguousarray(pred).astype(np.uint8))
    g = eng.to_device(np.ascontiguousarray(gt).astype(np.uint8))
    t = None if trimap is None else eng.to_device(np.ascontiguousarray(trimap, dtype=np.uint8))
    out = eng.empty(b, 14, dtype=torch.int64)
    eng.ctx.call("ggc_eval_counts", eng._stream(), b, h, w, p.data_ptr(), g.data_ptr(), None if t is None else t.data_ptr(),
                 int(boundary_width), out.data_ptr())
    return out.cpu().numpy()


def _bf1(n_pred: int, n_gt: int, n_both: int) -> float:
    prec = float(n_both / (n_pred + 1e-8))
    rec = float(n_both / (n_gt + 1e-8))
    return float(2 * prec * rec / (prec + rec + 1e-8))


def _from_counts(c: np.ndarray, n_pixels: int, with_boundary: bool) -> SegmentationMetrics:
    tp, fp, fn = int(c[0]), int(c[1]), int(c[2])
    tn = n_pixels - tp - fp - fn
    precision = float(tp / (tp + fp + 1e-8))
    recall = float(tp / (tp + fn + 1e-8))
    return SegmentationMetrics(
        iou=float(tp / (tp + fp + fn + 1e-8)), dice=float(2 * tp / (2 * tp + fp + fn + 1e-8)),
        precision=precision, recall=recall, f1=float(2 * precision * recall / (precision + recall + 1e-8)),
        pixel_accuracy=float((tp + tn) / (tp + tn + fp + fn + 1e-8)),
        boundary_f1=_bf1(int(c[3]), int(c[4]), int(c[5])) if with_boundary else 0.0)


def evaluate(pred: np.ndarray, gt: np.ndarray, boundary_width: int = 3, device="cuda") -> SegmentationMetrics:
    """Binary-mask metrics of one (H, W) pair — reference metrics.py:58-102."""
    c = _counts(pred, gt, None, boundary_width, device)[0]
    return _from_counts(c, int(np.asarray(pred).size), boundary_width > 0)


def boundary_f1(pred_2d: np.ndarray, gt_2d: np.ndarray, width: int = 3, device="cuda") -> float:
    """Alignment of predicted and GT boundaries, boundary = m - erode(m, ones(2*width+1)^2) — reference metrics.py:105-129."""
    c = _counts(pred_2d, gt_2d, None, width, device)[0]
    return _bf1(int(c[3]), int(c[4]), int(c[5]))


@dataclass
class TrimapMetrics:
    fg_recall: float
    fg_precision: float
    bg_recall: float
    bg_precision: float
    bg_contamination: float   # FG-labelled pixels that are actually BG
    unknown_fraction: float
    trimap_accuracy: float    # how much of the trimap matches the GT

    def __str__(self) -> str:
        return (f"FG_rec={self.fg_recall:.3f}  FG_prec={self.fg_precision:.3f}  BG_rec={self.bg_recall:.3f}  "
                f"BG_cont={self.bg_contamination:.3f}  Unk={self.unknown_fraction:.3f}  Acc={self.trimap_accuracy:.3f}")

    def as_dict(self) -> dict:
        return {k: round(v, 4) for k, v in self.__dict__.items()}


def evaluate_trimap(trimap: np.ndarray, gt_mask: np.ndarray, device="cuda") -> TrimapMetrics:
    """Predicted trimap {0 BG, 1 FG, 2 PROB_BG, 3 PROB_FG} against a binary GT mask — reference metrics.py:152-201.
    (gt_mask holds {0, 1}, as in the reference, whose accuracy term compares the raw mask values.)"""
    gt = np.asarray(gt_mask)
    c = _counts((np.asarray(trimap) == 1) | (np.asarray(trimap) == 3), gt, trimap, 0, device, binarize=False)[0]
    n = gt.size
    fg_tp, fg_fp, fg_fn, bg_tp, bg_fp, bg_fn, n_prob, n_match = (int(v) for v in c[6:14])
    return TrimapMetrics(
        fg_recall=float(fg_tp / (fg_tp + fg_fn + 1e-8)), fg_precision=float(fg_tp / (fg_tp + fg_fp + 1e-8)),
        bg_recall=float(bg_tp / (bg_tp + bg_fn + 1e-8)), bg_precision=float(bg_tp / (bg_tp + bg_fp + 1e-8)),
        bg_contamination=float(fg_fp / n), unknown_fraction=float(n_prob / n), trimap_accuracy=float(n_match / n))


def evaluate_batch(results: list[dict], device="cuda") -> dict:
    """Mean and std of IoU / Dice / BF1 over result dicts with "binary_mask" and "gt_mask" — reference metrics.py:204-229.
    Equally sized pairs are tallied in one device call."""
    all_iou, all_dice, all_bf1 = [], [], []
    by_shape: dict[tuple, list[int]] = {}
    for i, r in enumerate(results):
        by_shape.setdefault(np.asarray(r["binary_mask"]).shape, []).append(i)
    metrics: dict[int, SegmentationMetrics] = {}
    for shape, idx in by_shape.items():
        pred = np.stack([np.asarray(results[i]["binary_mask"]) for i in idx])
        gt = np.stack([np.asarray(results[i]["gt_mask"]) for i in idx])
        c = _counts(pred, gt, None, 3, device)
        for j, i in enumerate(idx):
            metrics[i] = _from_counts(c[j], int(np.prod(shape)), True)
    for i in range(len(results)):
        all_iou.append(metrics[i].iou); all_dice.append(metrics[i].dice); all_bf1.append(metrics[i].boundary_f1)
    return {"mean_iou": float(np.mean(all_iou)), "std_iou": float(np.std(all_iou)),
            "mean_dice": float(np.mean(all_dice)), "std_dice": float(np.std(all_dice)),
            "mean_bf1": float(np.mean(all_bf1)), "std_bf1": float(np.std(all_bf1)), "n": len(results)}


@dataclass
class MatteMetrics:
    """The four matte errors in their conventional units: sad = sum |a - g| / 1000, mse = mean (a - g)^2, grad = sum
    (m(a) - m(g))^2 / 1000, conn = sum |phi(a) - phi(g)| / 1000, alpha in [0, 1], over the n_pixels counted pixels."""
    sad: float
    mse: float
    grad: float
    conn: float
    n_pixels: int

    def __str__(self) -> str:
        return (f"SAD={self.sad:.4f}  MSE={self.mse:.6f}  Grad={self.grad:.4f}  Conn={self.conn:.4f}  "
                f"N={self.n_pixels}")

    def as_dict(self) -> dict:
        return {"sad": self.sad, "mse": self.mse, "grad": self.grad, "conn": self.conn, "n_pixels": self.n_pixels}


def matte_metrics_from_sums(sums, grad) -> MatteMetrics:
    """Raw sums of ggc_matte_errors (n, SAD in 1/255, SSE in 1/255^2, CONN in 1/2550; GRAD) -> MatteMetrics."""
    n, sad, sse, conn = (int(v) for v in sums)
    return MatteMetrics(sad=sad / 255.0 / 1000.0, mse=sse / 65025.0 / n if n else 0.0, grad=float(grad) / 1000.0,
                        conn=conn / 2550.0 / 1000.0, n_pixels=n)


def _matte_levels(alpha, what: str) -> np.ndarray:
    """uint8 levels as they are; floats in [0, 1] through pipeline.alpha_to_u8; anything else is a ValueError."""
    from .pipeline import alpha_to_u8
    a = np.asarray(alpha)
    if a.dtype == np.uint8:
        return a
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError(f"{what} must be uint8 levels or floats in [0, 1], got {a.dtype}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what} holds a value that is not finite")
    if a.size and (a.min() < 0.0 or a.max() > 1.0):
        raise ValueError(f"{what} must lie in [0, 1], got [{a.min():g}, {a.max():g}]")
    return alpha_to_u8(a)


def _matte_inputs(alpha, gt_alpha, region):
    """Checked (B,H,W) uint8 arrays of one call, and whether the input was a single (H,W) pair."""
    a, g = _matte_levels(alpha, "alpha"), _matte_levels(gt_alpha, "gt_alpha")
    if a.shape != g.shape:
        raise ValueError(f"shape mismatch: alpha {a.shape} vs gt_alpha {g.shape}")
    if a.ndim not in (2, 3):
        raise ValueError(f"mattes must be (H,W) or (B,H,W), got {a.shape}")
    r = None
    if region is not None:
        r = np.asarray(region)
        if r.shape != a.shape:
            raise ValueError(f"shape mismatch: region {r.shape} vs alpha {a.shape}")
        r = (r != 0).astype(np.uint8)
    single = a.ndim == 2
    if single:
        a, g, r = a[None], g[None], None if r is None else r[None]
    from ._engine import check_matte_eval_args
    check_matte_eval_args(a.shape, g.shape, None if r is None else r.shape)
    return a, g, r, single


def evaluate_matte(alpha, gt_alpha, region=None, device="cuda"):
    """SAD, MSE, gradient and connectivity error of a matte against the true matte (Rhemann et al., CVPR 2009), on the
    device (ggc_matte_errors, whose header entry states the definition).

    alpha, gt_alpha: one (H, W) pair -> MatteMetrics, or a (B, H, W) stack -> a list of them; uint8 levels, or floats
    in [0, 1], which are rounded to levels by pipeline.alpha_to_u8 (a float that is not finite or lies outside [0, 1] is
    a ValueError).  region: nonzero = counted, the unknown part of a trimap in the benchmarks; it restricts the sums
    only.  None counts every pixel."""
    a, g, r, single = _matte_inputs(alpha, gt_alpha, region)
    from ._engine import get_engine
    eng = get_engine(device)
    sums, grad, _ = eng.matte_errors(eng.to_device(np.ascontiguousarray(a)), eng.to_device(np.ascontiguousarray(g)),
                                     None if r is None else eng.to_device(np.ascontiguousarray(r)))
    sums, grad = sums.cpu().numpy(), grad.cpu().numpy()
    out = [matte_metrics_from_sums(sums[i], grad[i]) for i in range(len(a))]
    return out[0] if single else out


def evaluate_matte_batch(results: list[dict], device="cuda") -> dict:
    """Per-image MatteMetrics and their means over result dicts with "alpha" and "gt_alpha" (and optionally "region"),
    mirroring evaluate_batch.  Equally sized pairs with the same kind of region are scored in one device call."""
    groups: dict[tuple, list[int]] = {}
    for i, r in enumerate(results):
        groups.setdefault((np.asarray(r["alpha"]).shape, r.get("region") is not None), []).append(i)
    per: dict[int, MatteMetrics] = {}
    for (shape, has_region), idx in groups.items():
        a = np.stack([_matte_levels(results[i]["alpha"], "alpha") for i in idx])
        g = np.stack([_matte_levels(results[i]["gt_alpha"], "gt_alpha") for i in idx])
        reg = np.stack([np.asarray(results[i]["region"]) for i in idx]) if has_region else None
        for i, m in zip(idx, evaluate_matte(a, g, reg, device)):
            per[i] = m
    metrics = [per[i] for i in range(len(results))]
    out = {"metrics": metrics, "n": len(metrics)}
    for k in ("sad", "mse", "grad", "conn"):
        out[f"mean_{k}"] = float(np.mean([getattr(m, k) for m in metrics])) if metrics else 0.0
    return out


def noc_summary(ious, targets=(0.85, 0.90), max_clicks: int = 20) -> dict:
    """Number-of-clicks scores of interactive segmentation from IoU curves (pure host function).

    ious: (B, max_clicks + 1) IoU after 0, 1, ..., max_clicks clicks.  Per target t:
      noc[t] (B,) int    the first k with IoU >= t, or max_clicks if no k reaches t
      nof[t] int         the number of images that never reach t
    and mean_iou (max_clicks + 1,), the mean curve."""
    ious = np.asarray(ious, dtype=np.float64)
    max_clicks = int(max_clicks)
    if ious.ndim != 2 or ious.shape[1] != max_clicks + 1:
        raise ValueError(f"ious must be (B, {max_clicks + 1}), got {ious.shape}")
    noc, nof = {}, {}
    for t in targets:
        t = float(t)
        hit = ious >= t
        reached = hit.any(axis=1)
        noc[t] = np.where(reached, hit.argmax(axis=1), max_clicks).astype(np.int64)
        nof[t] = int((~reached).sum())
    mean = ious.mean(axis=0) if len(ious) else np.zeros(max_clicks + 1)
    return {"noc": noc, "nof": nof, "mean_iou": mean}
