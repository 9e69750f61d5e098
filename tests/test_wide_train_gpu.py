"""GPU: ResGCNNet training at widths above 128 (160 and 256): parameter gradients against the float64 CPU restatement of
test_train_resgcn_gpu.py on the hub graph and an edgeless graph, bit-identical repeated backward passes, the optimizer
step reaching the eval forward, and train.py --hidden 160 followed by inference.py on its checkpoint."""
import copy
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from test_train_resgcn_gpu import _batch, _loss, _model, _ref_forward

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("hidden", [160, 256])
def test_wide_parameter_gradients_match_float64_reference(gpu_ctx, hidden):
    m = _model(hidden, 2, seed=hidden).cuda().train()
    ref = copy.deepcopy(m).cpu().double().train()
    b = _batch(sizes=(600, 1, 9), seed=hidden, edgeless=(2,), hub=True)
    logits = m(b.to("cuda"))
    _loss(logits, b.to("cuda")).backward()
    ref_logits = _ref_forward(ref, b)
    _loss(ref_logits, b).backward()
    assert (logits.detach().double().cpu() - ref_logits.detach()).abs().max().item() < 1e-4
    for (k, p), (k2, q) in zip(m.named_parameters(), ref.named_parameters()):
        assert k == k2 and p.grad is not None, k
        g, r = p.grad.double().cpu(), q.grad
        rel = (g - r).norm().item() / max(r.norm().item(), 1e-12)
        analytic_zero = r.norm().item() < 1e-12 and g.abs().max().item() < 1e-7      # ctx.attn.bias (see the 128 test)
        assert rel <= 1e-4 or analytic_zero, (k, rel)


def test_wide_backward_passes_are_bit_identical(gpu_ctx):
    m = _model(256, 2, seed=11).cuda().train()
    b = _batch(sizes=(400, 1, 9), seed=11).to("cuda")
    grads = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        m.in_norm.norm.reset_running_stats()
        _loss(m(b), b).backward()
        grads.append([p.grad.cpu().numpy().copy() for p in m.parameters()])
    for (k, _), a, c in zip(m.named_parameters(), *grads):
        assert np.array_equal(a, c), k


def test_wide_optimizer_step_reaches_the_eval_forward(gpu_ctx):
    from gcn_grabcut.model import ResGCNNet
    m = _model(256, 2, seed=5).cuda()
    b = _batch(seed=5).to("cuda")
    before = m.eval()(b).clone()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    m.train()
    _loss(m(b), b).backward()
    opt.step()
    after = m.eval()(b)
    assert not torch.equal(before, after)
    fresh = ResGCNNet(hidden_channels=256, n_layers=2).cuda()
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(fresh.eval()(b), after)


def test_train_cli_at_160_then_inference(gpu_ctx, tmp_path):
    from PIL import Image
    from gcn_grabcut import synthetic_image
    for split, seeds in (("train", range(200, 204)), ("val", range(300, 302))):
        (tmp_path / "img" / split).mkdir(parents=True)
        (tmp_path / "msk" / split).mkdir(parents=True)
        for s in seeds:
            img, mask = synthetic_image(96, 128, s, return_mask=True)
            Image.fromarray(img[:, :, ::-1]).save(tmp_path / "img" / split / f"s{s}.png")
            Image.fromarray(mask * 255).save(tmp_path / "msk" / split / f"s{s}.png")
    ck = tmp_path / "ck"
    cmd = [sys.executable, str(ROOT / "train.py"), "--epochs", "1", "--hidden", "160", "--layers", "2",
           "--batch-size", "4", "--augment", "0", "--superpixels", "100",
           "--images_train", str(tmp_path / "img" / "train"), "--masks_train", str(tmp_path / "msk" / "train"),
           "--images_val", str(tmp_path / "img" / "val"), "--masks_val", str(tmp_path / "msk" / "val"),
           "--checkpoints", str(ck)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (ck / "final_model.pt").exists()
    out = tmp_path / "out"
    cmd = [sys.executable, str(ROOT / "inference.py"), "--image", str(tmp_path / "img" / "val" / "s300.png"),
           "--checkpoint", str(ck / "final_model.pt"), "--superpixels", "100", "--output", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert any(out.iterdir())
