"""ggc_alpha_matte on the MI355X: against the float64 restatement (tests/matte_ref.py), bit-for-bit batch independence,
exact locality, the grey-guide filter on grey images, a known soft edge, the pipeline and the command line."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from matte_ref import alpha_matte_ref, edge_band, soft_disk_scene

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _stream():
    from gcn_grabcut import _native
    return _native.current_stream(0)


def _call(ctx, bgr, binary, r, eps, want_rgba=False):
    """ggc_alpha_matte on (B,H,W,3) / (B,H,W) uint8 arrays -> alpha (B,H,W) f32 [, rgba] as device tensors."""
    bgr = torch.as_tensor(np.ascontiguousarray(bgr)).cuda()
    binary = torch.as_tensor(np.ascontiguousarray(binary)).cuda()
    b, h, w, _ = bgr.shape
    alpha = torch.empty(b, h, w, device="cuda")
    rgba = torch.empty(b, h, w, 4, dtype=torch.uint8, device="cuda") if want_rgba else None
    ctx.call("ggc_alpha_matte", _stream(), b, h, w, bgr.data_ptr(), binary.data_ptr(), r, eps, alpha.data_ptr(),
             None if rgba is None else rgba.data_ptr())
    return (alpha, rgba) if want_rgba else alpha


def _synthetic(h, w, seed):
    from gcn_grabcut.synthetic import synthetic_image
    return synthetic_image(h, w, seed, return_mask=True)


def _cases():
    rng = np.random.default_rng(5)
    out = []
    for (h, w) in ((1, 1), (1, 97), (83, 1), (37, 71), (65, 129)):
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        out.append((f"noise{h}x{w}", img, (rng.random((h, w)) < 0.5).astype(np.uint8)))
    img, gt = _synthetic(300, 400, 1)
    out.append(("synthetic300x400", img, gt))
    return out


@pytest.mark.parametrize("r", [1, 2, 4, 8, 16, 64])
@pytest.mark.parametrize("eps", [1e-2, 1e-4, 1e-5])
def test_device_matches_the_restatement(gpu_ctx, r, eps):
    for name, img, mask in _cases():
        got = _call(gpu_ctx, img[None], mask[None], r, eps)[0].cpu().numpy().astype(np.float64)
        err = np.abs(got - alpha_matte_ref(img, mask, r, eps)).max()
        assert err <= 2e-5, (name, r, eps, err)


def test_device_matches_the_restatement_on_windows_larger_than_the_image(gpu_ctx):
    rng = np.random.default_rng(8)
    for (h, w, r) in ((5, 3, 6), (20, 9, 30), (2, 2, 64)):
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        mask = (rng.random((h, w)) < 0.5).astype(np.uint8)
        for eps in (1e-2, 1e-5):
            got = _call(gpu_ctx, img[None], mask[None], r, eps)[0].cpu().numpy()
            assert np.abs(got - alpha_matte_ref(img, mask, r, eps)).max() <= 2e-5, (h, w, r, eps)


def test_device_matches_the_restatement_on_grabcut_masks(gpu_ctx):
    from gcn_grabcut import GrabCut
    for seed in (3, 4):
        img, _ = _synthetic(120, 160, seed)
        mask = GrabCut(img).run_with_bbox((30, 20, 100, 80)).astype(np.uint8)
        assert 0 < mask.sum() < mask.size
        for r, eps in ((4, 1e-4), (8, 1e-5), (2, 1e-2)):
            got = _call(gpu_ctx, img[None], mask[None], r, eps)[0].cpu().numpy()
            assert np.abs(got - alpha_matte_ref(img, mask, r, eps)).max() <= 2e-5


@pytest.mark.parametrize("r", [1, 4, 8])
def test_device_matches_the_restatement_full_hd(gpu_ctx, r):
    img, gt = _synthetic(1080, 1920, 6)
    got = _call(gpu_ctx, img[None], gt[None], r, 1e-4)[0].cpu().numpy()
    assert np.abs(got - alpha_matte_ref(img, gt, r, 1e-4)).max() <= 2e-5


def _mixed_batch(n=16, h=70, w=90):
    rng = np.random.default_rng(12)
    imgs, masks = [], []
    for k in range(n):
        if k % 4 == 0:
            img, m = _synthetic(h, w, 100 + k)
        elif k % 4 == 1:
            img, m = rng.integers(0, 256, (h, w, 3)).astype(np.uint8), (rng.random((h, w)) < 0.3).astype(np.uint8)
        elif k % 4 == 2:
            img, m = np.full((h, w, 3), 17 * k, np.uint8), np.full((h, w), k % 2, np.uint8)
        else:
            g = rng.integers(0, 256, (h, w)).astype(np.uint8)
            img, m = np.repeat(g[..., None], 3, axis=2), (g > 128).astype(np.uint8)
        imgs.append(img)
        masks.append(m)
    return np.stack(imgs), np.stack(masks)


def test_batch_equals_single_image_calls_bit_for_bit(gpu_ctx):
    imgs, masks = _mixed_batch()
    for r, eps in ((4, 1e-4), (9, 1e-5)):
        alpha, rgba = _call(gpu_ctx, imgs, masks, r, eps, want_rgba=True)
        again, rgba2 = _call(gpu_ctx, imgs, masks, r, eps, want_rgba=True)
        assert torch.equal(alpha, again) and torch.equal(rgba, rgba2)
        for k in range(len(imgs)):
            one, one_rgba = _call(gpu_ctx, imgs[k:k + 1], masks[k:k + 1], r, eps, want_rgba=True)
            assert torch.equal(one[0], alpha[k]) and torch.equal(one_rgba[0], rgba[k]), k
        a = alpha.cpu().numpy().astype(np.float64)
        rg = rgba.cpu().numpy()
        assert np.array_equal(rg[..., :3], imgs)
        assert np.abs(rg[..., 3] - 255.0 * a).max() <= 0.5 + 1e-4
        alpha_only = _call(gpu_ctx, imgs, masks, r, eps)
        assert torch.equal(alpha_only, alpha)


def test_any_nonzero_byte_is_foreground(gpu_ctx):
    imgs, masks = _mixed_batch(4)
    scaled = masks * np.array([255, 1, 7, 128], np.uint8)[:, None, None]
    assert torch.equal(_call(gpu_ctx, imgs, masks, 4, 1e-4), _call(gpu_ctx, imgs, scaled, 4, 1e-4))


@pytest.mark.parametrize("r", [1, 3, 8])
def test_far_from_the_edge_alpha_is_exactly_the_mask(gpu_ctx, r):
    imgs, masks = _mixed_batch(8, 130, 150)
    alpha = _call(gpu_ctx, imgs, masks, r, 1e-5).cpu().numpy()
    checked = 0
    for k in range(len(imgs)):
        far = ~edge_band(masks[k], 2 * r)
        assert np.array_equal(alpha[k][far], masks[k][far].astype(np.float32)), k
        checked += int(far.sum())
    assert checked > 0


@pytest.mark.parametrize("r,eps", [(2, 1e-2), (4, 3e-2), (8, 1e-2)])
def test_grey_image_agrees_with_the_grey_guided_filter(gpu_ctx, r, eps):
    from gcn_grabcut._engine import get_engine
    img, gt = _synthetic(96, 128, 21)
    grey = img[..., 1]
    alpha = _call(gpu_ctx, np.repeat(grey[..., None], 3, axis=2)[None], gt[None], r, eps)[0]
    eng = get_engine("cuda")
    guide = torch.as_tensor(grey[None] / np.float32(255.0), dtype=torch.float32).cuda()
    src = torch.as_tensor(gt[None], dtype=torch.float32).cuda()
    want = eng.guided_filter(guide, src, r, eps / 3.0)[0].clamp(0.0, 1.0)
    assert (alpha - want).abs().max().item() <= 1e-4


@pytest.mark.parametrize("r", [2, 4, 8])
@pytest.mark.parametrize("eps", [1e-2, 1e-4, 1e-5])
def test_matte_recovers_a_known_soft_edge(gpu_ctx, r, eps):
    # margin settled on the restatement first (test_matte_cpu.py::test_matte_recovers_a_known_soft_edge)
    for seed in (0, 1):
        img, alpha_true, mask = soft_disk_scene(120, 160, 40.0, 3.0, seed)
        band = edge_band(mask, 2 * r)
        a = _call(gpu_ctx, img[None], mask[None], r, eps)[0].cpu().numpy().astype(np.float64)
        assert np.abs(a - alpha_true)[band].sum() <= 0.8 * np.abs(mask - alpha_true)[band].sum()


# ---------------------------------------------------------------- arguments
@pytest.mark.parametrize("radius,eps", [(0, 1e-4), (65, 1e-4), (4, 0.0), (4, -1e-3)])
def test_entry_refuses_bad_arguments(gpu_ctx, radius, eps):
    from gcn_grabcut import _native
    imgs, masks = _mixed_batch(1, 8, 8)
    with pytest.raises(_native.GGCError) as e:
        _call(gpu_ctx, imgs, masks, radius, eps)
    assert e.value.code == -1                                  # GGC_E_INVALID_ARG
    from gcn_grabcut._engine import get_engine
    eng = get_engine("cuda")
    with pytest.raises(ValueError):
        eng.alpha_matte(torch.as_tensor(imgs).cuda(), torch.as_tensor(masks).cuda(), radius, eps)


def test_public_alpha_matte(gpu_ctx):
    from gcn_grabcut import alpha_matte
    img, gt = _synthetic(90, 110, 31)
    got = alpha_matte(img, gt.astype(bool), 5, 1e-3)
    assert got.dtype == np.float32 and got.shape == (90, 110)
    assert np.abs(got - alpha_matte_ref(img, gt, 5, 1e-3)).max() <= 2e-5
    gt[0, 0] = 2
    with pytest.raises(ValueError):
        alpha_matte(img, gt)


# ---------------------------------------------------------------- pipeline and command line
@pytest.fixture(scope="module")
def pipe():
    from helpers import seeded_state_dict
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig
    model, _ = seeded_state_dict(64, 3, seed=4)
    return GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=100), device="cuda:0")


@pytest.mark.parametrize("kw", [dict(chunks=1, grabcut_lanes=1), dict(chunks=1, grabcut_lanes=4),
                                dict(chunks=2, grabcut_lanes=4)])
def test_pipeline_matte_leaves_every_other_output_unchanged(pipe, kw):
    from gcn_grabcut._engine import get_engine
    from gcn_grabcut.synthetic import synthetic_batch
    bgr = torch.as_tensor(synthetic_batch(32, 72, 96, config_id=8)).cuda()
    plain = pipe.segment_batch_device(bgr, **kw)
    soft = pipe.segment_batch_device(bgr, matte=True, matte_radius=6, matte_eps=1e-3, **kw)
    torch.cuda.synchronize()
    assert "alpha" not in plain and "rgba_soft" not in plain
    for k in ("binary_mask", "trimap", "overlay", "rgba", "gc_mask"):
        assert torch.equal(plain[k], soft[k]), k
    eng = get_engine("cuda")
    want, want_rgba = eng.alpha_matte(bgr, soft["binary_mask"], 6, 1e-3, want_rgba=True)
    assert torch.equal(soft["alpha"], want) and torch.equal(soft["rgba_soft"], want_rgba)


def test_segment_and_segment_bbox_fill_the_matte(pipe):
    from gcn_grabcut import alpha_matte
    img, _ = _synthetic(80, 100, 41)
    r = pipe.segment(img, matte=True)
    assert r.alpha.shape == (80, 100) and r.rgba_soft.shape == (80, 100, 4)
    assert np.array_equal(r.alpha, alpha_matte(img, r.binary_mask))
    assert pipe.segment(img).alpha is None
    rb = pipe.segment_bbox(img, (20, 15, 60, 50), matte=True, matte_radius=3)
    assert np.array_equal(rb.alpha, alpha_matte(img, rb.binary_mask, 3))
    res = pipe.segment_batch([img, img[::-1].copy()], matte=True)
    assert all(np.array_equal(x.alpha, alpha_matte(x.image, x.binary_mask)) for x in res)


def test_inference_cli_writes_the_matte(tmp_path):
    from PIL import Image
    from helpers import seeded_state_dict
    from gcn_grabcut.synthetic import synthetic_image
    in_dir = tmp_path / "in"
    in_dir.mkdir()
    for k in range(2):
        Image.fromarray(synthetic_image(72, 96, 600 + k)[:, :, ::-1]).save(in_dir / f"im{k}.png")
    _, sd = seeded_state_dict(64, 3, seed=5)
    torch.save({"model": sd, "epoch": 1}, tmp_path / "ckpt.pt")

    def run(out, *extra):
        r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--input", str(in_dir), "--output", str(out),
                            "--checkpoint", str(tmp_path / "ckpt.pt"), "--superpixels", "100", "--max-size", "0", *extra],
                           cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return sorted(p.name for p in out.iterdir())

    assert run(tmp_path / "plain") == sorted(f"im{k}_{s}.png" for k in range(2) for s in ("mask", "overlay"))
    names = run(tmp_path / "soft", "--save", "mask", "alpha", "cutout", "--matte-radius", "3")
    assert names == sorted(f"im{k}_{s}.png" for k in range(2) for s in ("mask", "alpha", "cutout"))
    for k in range(2):
        mask = np.asarray(Image.open(tmp_path / "soft" / f"im{k}_mask.png"))
        alpha = Image.open(tmp_path / "soft" / f"im{k}_alpha.png")
        cut = Image.open(tmp_path / "soft" / f"im{k}_cutout.png")
        assert alpha.mode == "L" and alpha.size == (96, 72)
        assert cut.mode == "RGBA" and cut.size == (96, 72)
        a = np.asarray(alpha).astype(np.int64)
        assert np.abs(np.asarray(cut)[..., 3].astype(np.int64) - a).max() <= 1
        assert np.array_equal(np.asarray(mask), np.asarray(Image.open(tmp_path / "plain" / f"im{k}_mask.png")))
        far = ~edge_band(mask > 0, 6)
        assert np.array_equal(a[far], mask[far].astype(np.int64))
