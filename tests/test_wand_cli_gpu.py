"""The command line of the magic wand on the MI355X: inference.py --fg-wand / --bg-wand ... --save selection mask, run once
as a child process on a tiny image."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import wand_ref as ref
from helpers import seeded_state_dict

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_inference_writes_the_selection(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(4)
    img = np.array([60, 90, 120], np.uint8)[None, None, :] + rng.integers(0, 6, (60, 80, 3)).astype(np.uint8)   # BGR backdrop
    img[:, 50:] += 100                                                                                          # a second flat area
    img[15:45, 20:45] = rng.integers(0, 40, (30, 25, 3)).astype(np.uint8)                                       # a textured square
    img = np.ascontiguousarray(img)
    Image.fromarray(img[:, :, ::-1]).save(tmp_path / "x.png")
    model, sd = seeded_state_dict(32, 2, seed=8)
    torch.save({"model": sd, "epoch": 1}, tmp_path / "ckpt.pt")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--image", str(tmp_path / "x.png"), "--output", str(out),
                        "--checkpoint", str(tmp_path / "ckpt.pt"), "--superpixels", "60", "--min-area", "0",
                        "--bg-wand", "0,0 59,0", "--fg-wand", "59,79", "--wand-tolerance", "12", "--wand-connectivity", "4",
                        "--wand-sample", "3", "--save", "selection", "mask"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in out.iterdir()) == ["x_mask.png", "x_selection.png"]
    selection = np.asarray(Image.open(out / "x_selection.png"))
    _, want, counts = ref.wand_image(img, [(59, 79, 1), (0, 0, 0), (59, 0, 0)], 12, 4, 3)      # foreground seeds first
    assert np.array_equal(selection, want)
    right = np.zeros((60, 80), bool)
    right[:, 50:] = True
    assert np.array_equal(selection != 0, right) and counts.tolist() == [60 * 30, 60 * 50 - 30 * 25]
    mask = np.asarray(Image.open(out / "x_mask.png"))
    left = ref.selection(img, 0, 0, 12, 4, 3)
    assert mask.shape == (60, 80) and (mask[left] == 0).all() and (mask[right] == 255).all()   # hard constraints both ways
