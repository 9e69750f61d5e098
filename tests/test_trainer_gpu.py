"""GPU: Trainer end to end on synthetic images (prepare_dataset records), checkpoints with the reference's keys, the
best checkpoint through GCNGrabCutPipeline.segment, and train.py on an image/mask directory."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _samples(n, first_seed, h=96, w=128):
    from gcn_grabcut import synthetic_image
    out = []
    for i in range(n):
        img, mask = synthetic_image(h, w, first_seed + i, return_mask=True)
        out.append({"image": img, "gt_mask": mask, "name": f"s{first_seed + i}"})
    return out


def test_trainer_fits_and_checkpoints(gpu_ctx, tmp_path):
    from gcn_grabcut import GCNGrabCutPipeline, ResGCNNet, SuperpixelGraphConfig, TrainConfig, Trainer
    from gcn_grabcut.dataset import prepare_dataset
    sp = SuperpixelGraphConfig(n_segments=120)
    train = prepare_dataset(_samples(32, 100), sp, keep_segments=False)
    val = prepare_dataset(_samples(8, 900), sp, keep_segments=False)
    assert len(train) >= 28 and len(val) >= 6
    torch.manual_seed(0)
    model = ResGCNNet(hidden_channels=32, n_layers=2, dropout=0.1)
    cfg = TrainConfig(n_epochs=8, lr=3e-3, batch_size=8, scheduler="none", save_every=100, verbose=False)
    trainer = Trainer(model, cfg, device="cuda", save_dir=str(tmp_path / "ck"))
    untrained = trainer._eval_epoch(val)["score"]
    hist = trainer.fit(train, val)
    assert hist["train_loss"][-1] < hist["train_loss"][0]
    assert max(hist["val_score"]) > untrained
    for f in ("best_model.pt", "final_model.pt", "history.json"):
        assert (tmp_path / "ck" / f).exists(), f
    ck = torch.load(tmp_path / "ck" / "best_model.pt", weights_only=True)
    assert {"model", "optimizer", "epoch", "val_loss", "score", "config"} <= set(ck)
    h = json.loads((tmp_path / "ck" / "history.json").read_text())
    assert set(h) == {"train_loss", "val_loss", "val_acc", "val_iou_bg", "val_iou_unk", "val_iou_fg", "val_score", "lr"}
    best = ResGCNNet(hidden_channels=32, n_layers=2)
    best.load_state_dict(ck["model"])
    pipe = GCNGrabCutPipeline(best.cuda().eval(), sp_config=sp, device="cuda")
    res = pipe.segment(_samples(1, 5000)[0]["image"])
    assert res.binary_mask.shape == (96, 128)
    assert trainer.load("best_model.pt", weights_only=False) == ck["epoch"]


def test_train_cli_one_epoch(gpu_ctx, tmp_path):
    from PIL import Image
    for split, seeds in (("train", range(200, 206)), ("val", range(300, 303))):
        (tmp_path / "img" / split).mkdir(parents=True)
        (tmp_path / "msk" / split).mkdir(parents=True)
        for s in _samples(len(seeds), seeds[0]):
            Image.fromarray(s["image"][:, :, ::-1]).save(tmp_path / "img" / split / f"{s['name']}.png")
            Image.fromarray(s["gt_mask"] * 255).save(tmp_path / "msk" / split / f"{s['name']}.png")
    ck = tmp_path / "ck"
    cmd = [sys.executable, str(ROOT / "train.py"), "--epochs", "1", "--hidden", "32", "--layers", "2",
           "--batch-size", "4", "--augment", "0", "--superpixels", "100",
           "--images_train", str(tmp_path / "img" / "train"), "--masks_train", str(tmp_path / "msk" / "train"),
           "--images_val", str(tmp_path / "img" / "val"), "--masks_val", str(tmp_path / "msk" / "val"),
           "--checkpoints", str(ck)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (ck / "final_model.pt").exists() and (ck / "history.json").exists()
    r = subprocess.run([sys.executable, str(ROOT / "train.py"), "--model", "gat"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "inference-only" in (r.stdout + r.stderr)
