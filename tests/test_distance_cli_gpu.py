"""The command lines of the mask modifiers on the MI355X: inference.py --modify ... --save modified, and matte.py --mask
... --band, each run once as a child process."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import distance_ref as ref
from helpers import seeded_state_dict

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def run(script, *args, cwd):
    r = subprocess.run([sys.executable, str(ROOT / script), *map(str, args)], cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def test_inference_writes_the_modified_mask_and_nothing_else_changes(tmp_path):
    from PIL import Image
    from gcn_grabcut.synthetic import synthetic_image
    img = synthetic_image(150, 200, 30003)
    Image.fromarray(img[:, :, ::-1]).save(tmp_path / "x.png")
    model, sd = seeded_state_dict(32, 2, seed=8)
    torch.save({"model": sd, "epoch": 1}, tmp_path / "ckpt.pt")
    common = ["--image", tmp_path / "x.png", "--checkpoint", tmp_path / "ckpt.pt", "--superpixels", "100", "--max-size", "100",
              "--min-area", "0"]
    plain, out = tmp_path / "plain", tmp_path / "out"
    run("inference.py", *common, "--output", plain, cwd=tmp_path)
    assert sorted(p.name for p in plain.iterdir()) == ["x_mask.png", "x_overlay.png"]          # without the flags: what it was
    run("inference.py", *common, "--output", out, "--modify", "shrink:2", "--modify", "grow:2", "--save", "mask", "modified",
        cwd=tmp_path)
    assert sorted(p.name for p in out.iterdir()) == ["x_mask.png", "x_modified.png"]
    mask = np.asarray(Image.open(out / "x_mask.png"))
    assert np.array_equal(mask, np.asarray(Image.open(plain / "x_mask.png"))) and mask.any()
    modified = np.asarray(Image.open(out / "x_modified.png"))
    assert np.array_equal(modified, 255 * ref.modify(mask, ref.OPEN, 4))                       # open_mask of the run's mask


def test_matte_from_a_mask_and_a_band(tmp_path):
    from PIL import Image
    from gcn_grabcut.synthetic import synthetic_image
    img, gt = synthetic_image(48, 64, 30002, return_mask=True)
    Image.fromarray(img[:, :, ::-1]).save(tmp_path / "x.png")
    Image.fromarray(gt * np.uint8(255)).save(tmp_path / "x_mask.png")
    run("matte.py", "--image", tmp_path / "x.png", "--mask", tmp_path / "x_mask.png", "--band", "3:5", "--output", tmp_path / "out",
        cwd=tmp_path)
    alpha = np.asarray(Image.open(tmp_path / "out" / "x_alpha.png"))
    tri = ref.modify(gt, ref.TRIMAP, 9, 25)
    assert (tri == 128).any() and np.all(alpha[tri == 255] == 255) and np.all(alpha[tri == 0] == 0)
