"""CPU: FocalLoss / LabelSmoothingCE / TrimapLoss and their gradients w.r.t. the logits against values the reference's
own losses.py produced (tests/golden/reference_losses.npz, written by make_golden_reference_losses.py)."""
from pathlib import Path

import numpy as np
import pytest
import torch

from gcn_grabcut import FocalLoss, LabelSmoothingCE, TrimapLoss

G = np.load(Path(__file__).resolve().parent / "golden" / "reference_losses.npz")
T = {k: torch.from_numpy(G[k]) for k in ("logits", "labels", "area", "fg_ratio", "batch", "class_weight")}
W = T["class_weight"]

CASES = {
    "focal": (lambda: FocalLoss(gamma=2.0, weight=W), {}),
    "focal_noweight": (lambda: FocalLoss(gamma=2.5), {}),
    "smooth_ce": (lambda: LabelSmoothingCE(smoothing=0.1, weight=W), {}),
    "smooth_ce_noweight": (lambda: LabelSmoothingCE(smoothing=0.2), {}),
    "trimap_full": (lambda: TrimapLoss(gamma=2.0, weight=W, dice_weight=0.5), ("area", "fg_ratio", "batch")),
    "trimap_nobatch": (lambda: TrimapLoss(gamma=2.0, weight=W, dice_weight=0.5), ("area", "fg_ratio")),
    "trimap_labels_target": (lambda: TrimapLoss(gamma=2.0, weight=W, dice_weight=0.7), ("area", "batch")),
    "trimap_no_area": (lambda: TrimapLoss(gamma=2.0, dice_weight=0.5), ("fg_ratio", "batch")),
    "trimap_gamma0": (lambda: TrimapLoss(gamma=0.0, weight=W, dice_weight=0.5), ("area", "fg_ratio", "batch")),
    "trimap_no_dice": (lambda: TrimapLoss(gamma=2.0, weight=W, dice_weight=0.0), ("area",)),
    "trimap_unweighted_area": (lambda: TrimapLoss(gamma=2.0, weight=W, dice_weight=0.5, area_weighted=False),
                               ("area", "fg_ratio", "batch")),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_loss_and_logit_gradient_match_reference(name):
    make, keys = CASES[name]
    logits = T["logits"].clone().requires_grad_(True)
    loss = make()(logits, T["labels"], **{k: T[k] for k in keys})
    loss.backward()
    want, want_g = float(G[f"{name}/loss"]), G[f"{name}/grad"]
    assert abs(loss.item() - want) <= 1e-12 * (1 + abs(want)), (loss.item(), want)
    np.testing.assert_allclose(logits.grad.numpy(), want_g, rtol=1e-10, atol=1e-13)


def test_golden_covers_every_case():
    assert {k.split("/")[0] for k in G.files if "/" in k} == set(CASES)


def test_per_graph_dice_is_independent_of_node_order_within_the_batch_vector():
    """The Dice sums are per graph: interleaving the graphs' nodes changes nothing but the summation order."""
    perm = torch.randperm(T["logits"].size(0), generator=torch.Generator().manual_seed(3))
    crit = TrimapLoss(gamma=2.0, weight=W, dice_weight=0.5)
    a = crit(T["logits"], T["labels"], area=T["area"], fg_ratio=T["fg_ratio"], batch=T["batch"])
    b = crit(T["logits"][perm], T["labels"][perm], area=T["area"][perm], fg_ratio=T["fg_ratio"][perm],
             batch=T["batch"][perm])
    assert abs(a.item() - b.item()) < 1e-12
