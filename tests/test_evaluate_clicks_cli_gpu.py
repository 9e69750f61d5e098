"""evaluate_clicks.py end to end on a directory of synthetic PNGs and a random-weight checkpoint."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import seeded_state_dict

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _write_set(tmp_path, shapes):
    from PIL import Image
    from gcn_grabcut.synthetic import synthetic_image
    imgs, masks = tmp_path / "images", tmp_path / "masks"
    imgs.mkdir()
    masks.mkdir()
    for i, (h, w) in enumerate(shapes):
        img, gt = synthetic_image(h, w, 300 + i, return_mask=True)
        Image.fromarray(img[:, :, ::-1]).save(imgs / f"im{i}.png")
        Image.fromarray(gt.astype(np.uint8) * 255).save(masks / f"im{i}.png")
    return imgs, masks


def _checkpoint(tmp_path):
    _, sd = seeded_state_dict(32, 2, seed=21)
    torch.save({"model": sd, "epoch": 1}, tmp_path / "ckpt.pt")
    return tmp_path / "ckpt.pt"


def _run(args, cwd):
    return subprocess.run([sys.executable, str(ROOT / "evaluate_clicks.py"), *map(str, args)], cwd=cwd,
                          capture_output=True, text=True, timeout=900)


def test_cli_end_to_end(tmp_path):
    imgs, masks = _write_set(tmp_path, [(90, 120)] * 3 + [(100, 80)] * 2)      # two shapes: two batches
    out = tmp_path / "noc.json"
    r = _run(["--images", imgs, "--masks", masks, "--checkpoint", _checkpoint(tmp_path), "--superpixels", "60",
              "--max-clicks", "4", "--targets", "0.85", "0.9", "--hint-radius", "3", "--batch", "2", "--json", out],
             tmp_path)
    assert r.returncode == 0, r.stderr
    assert "NoC@0.85" in r.stdout and "NoF@0.90" in r.stdout and "@4=" in r.stdout
    doc = json.loads(out.read_text())
    assert set(doc) >= {"config", "noc", "nof", "mean_iou", "images"}
    assert set(doc["noc"]) == set(doc["nof"]) == {"0.85", "0.90"}
    assert len(doc["mean_iou"]) == 5 and len(doc["images"]) == 5
    assert sorted(im["name"] for im in doc["images"]) == [f"im{i}" for i in range(5)]
    for im in doc["images"]:
        assert len(im["ious"]) == 5 and len(im["clicks"]) <= 4
        assert all(len(c) == 3 and c[2] in (0, 1) for c in im["clicks"])
        assert set(im["noc"]) == {"0.85", "0.90"} and all(0 <= v <= 4 for v in im["noc"].values())
    assert np.allclose(doc["mean_iou"], np.mean([im["ious"] for im in doc["images"]], axis=0))


def test_cli_refuses_a_mask_of_another_size(tmp_path):
    from PIL import Image
    imgs, masks = _write_set(tmp_path, [(60, 80)] * 2)
    Image.fromarray(np.zeros((60, 81), np.uint8)).save(masks / "im1.png")
    r = _run(["--images", imgs, "--masks", masks, "--checkpoint", _checkpoint(tmp_path), "--max-clicks", "2"], tmp_path)
    assert r.returncode != 0
    assert "im1.png" in r.stderr and "mask" in r.stderr
