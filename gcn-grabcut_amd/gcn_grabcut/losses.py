"""
Training objectives for the trimap network — the arithmetic of the reference's losses.py.

`FocalLoss`, `LabelSmoothingCE` and `TrimapLoss` compute what the reference modules compute (same arguments, same
formulas, pinned against values the reference itself produced: tests/golden/reference_losses.npz).  They are plain
torch and run on any device.  One difference in mechanism, none in value: the per-graph sums of TrimapLoss's Dice
term use a segmented reduction instead of `index_add_`, whose float atomics on the GPU would make the loss — and every
gradient — change in the last bits from run to run.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .model import CLASS_FG, CLASS_UNK


def _per_graph_sums(vals: list, batch: torch.Tensor) -> list:
    """Sum of each tensor in `vals` over the nodes of every graph (graph ids 0..max(batch)), in a fixed order."""
    n_graphs = int(batch.max().item()) + 1
    order = torch.argsort(batch, stable=True)
    lengths = torch.bincount(batch, minlength=n_graphs)
    return [torch.segment_reduce(v[order], "sum", lengths=lengths) for v in vals]


class FocalLoss(nn.Module):
    """mean over nodes of (1 - p_t)^gamma * CE, p_t = exp(-CE) (Lin et al. 2017); CE optionally class-weighted."""

    def __init__(self, gamma: float = 2.0, weight: Optional[torch.Tensor] = None):
        super().__init__()
        self.gamma = gamma
        self.weight = weight

    def forward(self, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        ce = F.cross_entropy(logits, labels, weight=self.weight, reduction="none")
        return ((1.0 - torch.exp(-ce)) ** self.gamma * ce).mean()


class LabelSmoothingCE(nn.Module):
    """Cross-entropy against a smoothed target: 1 - s on the label, s / (K - 1) on every other class."""

    def __init__(self, smoothing: float = 0.1, weight: Optional[torch.Tensor] = None):
        super().__init__()
        self.smoothing = smoothing
        self.weight = weight

    def forward(self, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        k = logits.size(-1)
        logp = F.log_softmax(logits, dim=-1)
        target = torch.full_like(logp, self.smoothing / (k - 1)).detach()
        target.scatter_(1, labels.unsqueeze(1), 1.0 - self.smoothing)
        per_node = -(target * logp).sum(dim=-1)
        if self.weight is not None:
            per_node = per_node * self.weight[labels]
        return per_node.mean()


class TrimapLoss(nn.Module):
    """
    Area-weighted focal CE over {BG, UNKNOWN, FG} plus `dice_weight` x a soft Dice term on the expected foreground
    coverage p = P(FG) + P(UNKNOWN) / 2, computed per graph and averaged over graphs when `batch` is given.

    Classification: per-node (1 - p_t)^gamma * CE with p_t = exp(-min(CE, 30)) taken from the DETACHED CE (plain CE
    when gamma == 0); with `area` and `area_weighted`, each node is weighted by area * N / max(sum area, eps).
    Dice target: `fg_ratio` when given, else 1 for FG, 1/2 for UNKNOWN, 0 for BG; weights `area` (or 1).
    """

    def __init__(self, gamma: float = 2.0, weight: Optional[torch.Tensor] = None, dice_weight: float = 0.5,
                 area_weighted: bool = True, eps: float = 1e-6):
        super().__init__()
        self.gamma = gamma
        self.weight = weight
        self.dice_weight = dice_weight
        self.area_weighted = area_weighted
        self.eps = eps

    def forward(self, logits: torch.Tensor, labels: torch.Tensor, area: Optional[torch.Tensor] = None,
                fg_ratio: Optional[torch.Tensor] = None, batch: Optional[torch.Tensor] = None) -> torch.Tensor:
        ce = F.cross_entropy(logits, labels, weight=self.weight, reduction="none")
        if self.gamma > 0:
            p_t = torch.exp(-ce.detach().clamp(max=30.0))
            per_node = (1.0 - p_t) ** self.gamma * ce
        else:
            per_node = ce
        if area is not None and self.area_weighted:
            a = area.to(per_node.dtype)
            per_node = per_node * (a * (a.numel() / a.sum().clamp(min=self.eps)))
        cls_loss = per_node.mean()
        if self.dice_weight <= 0:
            return cls_loss

        probs = F.softmax(logits, dim=-1)
        pred = probs[:, CLASS_FG] + 0.5 * probs[:, CLASS_UNK]
        if fg_ratio is not None:
            target = fg_ratio.to(pred.dtype)
        else:
            target = (labels == CLASS_FG).to(pred.dtype) + 0.5 * (labels == CLASS_UNK).to(pred.dtype)
        a = torch.ones_like(pred) if area is None else area.to(pred.dtype)
        terms = [a * pred * target, a * pred, a * target]
        if batch is None:
            inter, sum_p, sum_t = (t.sum() for t in terms)
        else:
            inter, sum_p, sum_t = _per_graph_sums(terms, batch)
        dice = (1.0 - (2.0 * inter + self.eps) / (sum_p + sum_t + self.eps)).mean()
        return cls_loss + self.dice_weight * dice
