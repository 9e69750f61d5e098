"""
Generates tests/golden/reference_losses.npz by running the REFERENCE's own losses.py (FocalLoss, LabelSmoothingCE,
TrimapLoss) on fixed inputs.

Run in the build container only (the reference never travels), with the main interpreter (torch-CPU):
    python3 tests/golden/make_golden_reference_losses.py
The reference package is loaded by path with the same placeholders as make_golden_reference_torch.py (cv2 and the
scikit-image names imported at module level; nothing in them is called).  losses.py needs model.py only for the class
ids.

Recorded, in float64, for each case: the loss value and its gradient with respect to the logits.  Inputs: 3 graphs
(37, 1 and 22 nodes; the second is a single node), logits spread wide enough that the clamp at CE = 30 of TrimapLoss
is exercised by one node, labels with all three classes, positive areas, fg_ratio in [0, 1].
"""
import importlib.util
import pathlib
import sys
import types

import numpy as np
import torch

HERE = pathlib.Path(__file__).resolve().parent
REF = pathlib.Path("/root/reference/src/gcn_grabcut")


def placeholder(name, *attrs):
    m = types.ModuleType(name)
    for a in attrs:
        setattr(m, a, None)
    sys.modules[name] = m
    return m


placeholder("cv2")
sk = placeholder("skimage")
sk.segmentation = placeholder("skimage.segmentation", "slic", "find_boundaries", "mark_boundaries")
sk.color = placeholder("skimage.color", "rgb2lab", "rgb2hsv")
sk.measure = placeholder("skimage.measure", "regionprops")
pkg = types.ModuleType("refpkg")
pkg.__path__ = [str(REF)]
sys.modules["refpkg"] = pkg


def load(name):
    spec = importlib.util.spec_from_file_location(f"refpkg.{name}", REF / f"{name}.py")
    m = importlib.util.module_from_spec(spec)
    sys.modules[f"refpkg.{name}"] = m
    spec.loader.exec_module(m)
    return m


load("graph_builder")
load("model")
losses = load("losses")

g = torch.Generator().manual_seed(1234)
sizes = [37, 1, 22]
n = sum(sizes)
logits = torch.randn(n, 3, generator=g, dtype=torch.float64) * 3.0
logits[5] = torch.tensor([40.0, -5.0, -3.0], dtype=torch.float64)     # CE > 30 if the label is not BG
labels = torch.randint(0, 3, (n,), generator=g)
labels[5] = 2
area = torch.rand(n, generator=g, dtype=torch.float64) * 0.01 + 1e-4
fg_ratio = torch.rand(n, generator=g, dtype=torch.float64)
batch = torch.cat([torch.full((s,), i, dtype=torch.long) for i, s in enumerate(sizes)])
weight = torch.tensor([1.5, 0.8, 1.5], dtype=torch.float64)

CASES = {
    "focal": (lambda: losses.FocalLoss(gamma=2.0, weight=weight), {}),
    "focal_noweight": (lambda: losses.FocalLoss(gamma=2.5), {}),
    "smooth_ce": (lambda: losses.LabelSmoothingCE(smoothing=0.1, weight=weight), {}),
    "smooth_ce_noweight": (lambda: losses.LabelSmoothingCE(smoothing=0.2), {}),
    "trimap_full": (lambda: losses.TrimapLoss(gamma=2.0, weight=weight, dice_weight=0.5),
                    dict(area=area, fg_ratio=fg_ratio, batch=batch)),
    "trimap_nobatch": (lambda: losses.TrimapLoss(gamma=2.0, weight=weight, dice_weight=0.5),
                       dict(area=area, fg_ratio=fg_ratio)),
    "trimap_labels_target": (lambda: losses.TrimapLoss(gamma=2.0, weight=weight, dice_weight=0.7),
                             dict(area=area, batch=batch)),
    "trimap_no_area": (lambda: losses.TrimapLoss(gamma=2.0, dice_weight=0.5), dict(fg_ratio=fg_ratio, batch=batch)),
    "trimap_gamma0": (lambda: losses.TrimapLoss(gamma=0.0, weight=weight, dice_weight=0.5),
                      dict(area=area, fg_ratio=fg_ratio, batch=batch)),
    "trimap_no_dice": (lambda: losses.TrimapLoss(gamma=2.0, weight=weight, dice_weight=0.0), dict(area=area)),
    "trimap_unweighted_area": (lambda: losses.TrimapLoss(gamma=2.0, weight=weight, dice_weight=0.5, area_weighted=False),
                               dict(area=area, fg_ratio=fg_ratio, batch=batch)),
}

out = {"torch_version": np.array(torch.__version__), "logits": logits.numpy(), "labels": labels.numpy(),
       "area": area.numpy(), "fg_ratio": fg_ratio.numpy(), "batch": batch.numpy(), "class_weight": weight.numpy()}
for name, (make, kw) in CASES.items():
    lg = logits.clone().requires_grad_(True)
    loss = make()(lg, labels, **kw)
    loss.backward()
    out[f"{name}/loss"] = np.array(loss.item())
    out[f"{name}/grad"] = lg.grad.numpy()
np.savez_compressed(HERE / "reference_losses.npz", **out)
print(f"wrote {HERE / 'reference_losses.npz'}: {len(CASES)} cases")
