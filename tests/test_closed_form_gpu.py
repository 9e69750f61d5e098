"""ggc_closed_form_matte on the MI355X: known pixels exact, a residual certificate recomputed in float64 on the host,
agreement with the restatement (tests/closed_form_ref.py), bit-for-bit batch independence, the quality margin settled
in test_closed_form_cpu.py, argument checks, the pipeline and the command line."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from closed_form_ref import band_sad, pcg, residual_norms, strand_scene, unknown_band
from matte_ref import alpha_matte_ref, edge_band, soft_disk_scene
from test_closed_form_cpu import DEFAULTS, QUALITY, TAU

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _stream():
    from gcn_grabcut import _native
    return _native.current_stream(0)


def _call(ctx, bgr, binary, r=1, eps=1e-5, band=1, max_iter=500, tol=1e-4):
    """ggc_closed_form_matte on (B,H,W,3) / (B,H,W) uint8 arrays -> dict of device tensors."""
    bgr = torch.as_tensor(np.ascontiguousarray(bgr)).cuda()
    binary = torch.as_tensor(np.ascontiguousarray(binary)).cuda()
    b, h, w, _ = bgr.shape
    out = dict(alpha=torch.empty(b, h, w, device="cuda"), rgba=torch.empty(b, h, w, 4, dtype=torch.uint8, device="cuda"),
               raw=torch.empty(b, h, w, dtype=torch.float64, device="cuda"),
               iters=torch.empty(b, dtype=torch.int32, device="cuda"),
               rel=torch.empty(b, dtype=torch.float64, device="cuda"))
    ctx.call("ggc_closed_form_matte", _stream(), b, h, w, bgr.data_ptr(), binary.data_ptr(), r, eps, band, max_iter, tol,
             out["alpha"].data_ptr(), out["rgba"].data_ptr(), out["raw"].data_ptr(), out["iters"].data_ptr(),
             out["rel"].data_ptr())
    torch.cuda.synchronize()
    return out


def _synthetic(h, w, seed):
    from gcn_grabcut.synthetic import synthetic_image
    return synthetic_image(h, w, seed, return_mask=True)


def _grabcut_case(h, w, seed):
    from gcn_grabcut import GrabCut
    img, _ = _synthetic(h, w, seed)
    mask = GrabCut(img).run_with_bbox((w // 5, h // 6, 3 * w // 5, 2 * h // 3)).astype(np.uint8)
    assert 0 < mask.sum() < mask.size
    return img, mask


def _cases():
    out = [("disk0", *soft_disk_scene(120, 160, 40.0, 3.0, 0)[::2]), ("strands0", *strand_scene(120, 160, seed=0)[::2])]
    for seed, (h, w) in ((3, (96, 128)), (4, (77, 131))):
        out.append((f"grabcut{seed}", *_grabcut_case(h, w, seed)))
    img, gt = _synthetic(53, 67, 9)
    out.append(("odd53x67", img, gt))
    return out


@pytest.mark.parametrize("r", [1, 2, 4])
@pytest.mark.parametrize("band", [1, 3])
def test_known_pixels_exact_and_residual_certificate(gpu_ctx, r, band):
    tol, eps, max_iter = 1e-4, 1e-5, 2000
    for name, img, mask in _cases():
        o = _call(gpu_ctx, img[None], mask[None], r, eps, band, max_iter, tol)
        raw = o["raw"][0].cpu().numpy()
        alpha = o["alpha"][0].cpu().numpy()
        U = unknown_band(mask, band)
        m = mask.astype(np.float64)
        assert np.array_equal(raw[~U], m[~U]) and np.array_equal(alpha[~U], m[~U].astype(np.float32)), name
        assert np.array_equal(alpha, np.clip(raw, 0.0, 1.0).astype(np.float32)), name
        iters, rel = int(o["iters"][0]), float(o["rel"][0])
        assert 1 <= iters <= max_iter, (name, iters)
        res, res0 = residual_norms(img, mask, raw, r, eps, band)
        assert res <= 2.0 * tol * res0, (name, res / res0)
        assert abs(rel - res / res0) <= 0.1 * (res / res0), (name, rel, res / res0)
        assert rel <= tol, (name, rel)


@pytest.mark.parametrize("r", [1, 2, 4])
def test_agrees_with_the_restatement(gpu_ctx, r):
    d = DEFAULTS
    for name, img, mask in _cases():
        got = _call(gpu_ctx, img[None], mask[None], r, d["eps"], d["band"], d["max_iter"], d["tol"])["alpha"][0]
        want, _, rel = pcg(img, mask, r, d["eps"], d["band"], 20000, 1e-12)
        err = np.abs(got.cpu().numpy().astype(np.float64) - np.clip(want, 0.0, 1.0)).max()
        assert err <= TAU, (name, r, err)


def _mixed_batch(h=70, w=90):
    rng = np.random.default_rng(12)
    imgs, masks = [], []
    for k in range(10):
        img, m = _synthetic(h, w, 100 + k)
        if k == 1:
            m = np.zeros((h, w), np.uint8)                       # all background: U empty
        elif k == 2:
            m = np.ones((h, w), np.uint8)                        # all foreground
        elif k == 3:
            m = np.zeros((h, w), np.uint8)
            m[h // 2, w // 3] = 1                                # one-pixel object
        elif k == 4:
            img = np.zeros((h, w, 3), np.uint8)
            img[..., 1] = rng.integers(0, 256, (h, w))
            m = (rng.random((h, w)) < 0.5).astype(np.uint8)     # noise: every pixel within band 2 of an edge
        elif k == 5:
            img = np.full((h, w, 3), 90, np.uint8)              # flat colour
        imgs.append(img)
        masks.append(m)
    return np.stack(imgs), np.stack(masks)


def test_batch_equals_single_image_calls_bit_for_bit(gpu_ctx):
    imgs, masks = _mixed_batch()
    assert unknown_band(masks[4], 2).all()
    for r, band in ((1, 2), (2, 1)):
        full = _call(gpu_ctx, imgs, masks, r, 1e-5, band, 300, 1e-5)
        again = _call(gpu_ctx, imgs, masks, r, 1e-5, band, 300, 1e-5)
        for k in full:
            assert torch.equal(full[k], again[k]), k
        for j in range(len(imgs)):
            one = _call(gpu_ctx, imgs[j:j + 1], masks[j:j + 1], r, 1e-5, band, 300, 1e-5)
            for k in full:
                assert torch.equal(one[k][0], full[k][j]), (j, k)
        it = full["iters"].cpu().numpy()
        assert it[1] == 0 and it[2] == 0 and it[3] > 0
        if band == 2:
            assert it[4] == 0 and torch.equal(full["raw"][4], torch.as_tensor(masks[4], dtype=torch.float64).cuda())
        rg = full["rgba"].cpu().numpy()
        a = full["alpha"].cpu().numpy().astype(np.float64)
        assert np.array_equal(rg[..., :3], imgs)
        assert np.array_equal(rg[..., 3], np.floor(np.clip(full["raw"].cpu().numpy(), 0, 1) * 255.0 + 0.5).astype(np.uint8))
        assert np.abs(rg[..., 3] - 255.0 * a).max() <= 0.5 + 1e-4


def test_any_nonzero_byte_is_foreground(gpu_ctx):
    imgs, masks = _mixed_batch()
    scaled = masks * np.uint8(200)
    a, b = _call(gpu_ctx, imgs[:4], masks[:4]), _call(gpu_ctx, imgs[:4], scaled[:4])
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name,scene", [("disk0", soft_disk_scene(120, 160, 40.0, 3.0, 0)),
                                        ("disk1", soft_disk_scene(120, 160, 40.0, 3.0, 1)),
                                        ("strands0", strand_scene(120, 160, seed=0))])
def test_closed_form_beats_the_guided_matte_on_soft_edges(gpu_ctx, name, scene):
    # margin settled on the restatement first (test_closed_form_cpu.py::test_closed_form_beats_the_guided_matte_...)
    from gcn_grabcut import closed_form_matte
    img, alpha_true, mask = scene
    region = edge_band(mask, 8)
    a = closed_form_matte(img, mask)
    guided = band_sad(alpha_matte_ref(img, mask, 4, 1e-4), alpha_true, region)
    assert band_sad(a, alpha_true, region) <= QUALITY * guided, name


# ---------------------------------------------------------------- arguments
@pytest.mark.parametrize("args,code", [((0, 1e-5, 1, 10, 1e-4), -1), ((9, 1e-5, 1, 10, 1e-4), -1),
                                       ((1, 0.0, 1, 10, 1e-4), -1), ((1, 1e-5, -1, 10, 1e-4), -1),
                                       ((1, 1e-5, 1, 0, 1e-4), -1), ((1, 1e-5, 1, 10, 0.0), -1),
                                       ((1, 1e-5, 1, 10, 1.0), -1), ((5, 1e-5, 1, 10, 1e-4), -2)])
def test_entry_refuses_bad_arguments(gpu_ctx, args, code):
    from gcn_grabcut import _native
    from gcn_grabcut._engine import get_engine
    imgs, masks = _mixed_batch(10, 12)
    with pytest.raises(_native.GGCError) as e:
        _call(gpu_ctx, imgs[:1], masks[:1], *args)
    assert e.value.code == code
    eng = get_engine("cuda")
    with pytest.raises(ValueError):
        eng.closed_form_matte(torch.as_tensor(imgs[:1]).cuda(), torch.as_tensor(masks[:1]).cuda(), *args)


def test_entry_refuses_a_call_without_outputs_and_accepts_an_empty_batch(gpu_ctx):
    from gcn_grabcut import _native
    imgs, masks = _mixed_batch(10, 12)
    bgr, m = torch.as_tensor(imgs[:1]).cuda(), torch.as_tensor(masks[:1]).cuda()
    with pytest.raises(_native.GGCError) as e:
        gpu_ctx.call("ggc_closed_form_matte", _stream(), 1, 10, 12, bgr.data_ptr(), m.data_ptr(), 1, 1e-5, 1, 10, 1e-4,
                     None, None, None, None, None)
    assert e.value.code == -1
    out = torch.empty(1, device="cuda")
    gpu_ctx.call("ggc_closed_form_matte", _stream(), 0, 10, 12, None, None, 1, 1e-5, 1, 10, 1e-4, out.data_ptr(), None,
                 None, None, None)


def test_public_closed_form_matte(gpu_ctx):
    from gcn_grabcut import closed_form_matte
    img, alpha_true, mask = strand_scene(120, 160, seed=0)
    a, it, rel = closed_form_matte(img, mask.astype(bool), return_info=True)
    assert a.dtype == np.float32 and a.shape == (120, 160) and 1 <= it <= 500 and rel <= 1e-4
    assert np.array_equal(a, closed_form_matte(img, mask))
    mask[0, 0] = 2
    with pytest.raises(ValueError):
        closed_form_matte(img, mask)


# ---------------------------------------------------------------- pipeline and command line
@pytest.fixture(scope="module")
def pipe():
    from helpers import seeded_state_dict
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig
    model, _ = seeded_state_dict(64, 3, seed=4)
    return GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=100), device="cuda:0")


@pytest.mark.parametrize("kw", [dict(chunks=1, grabcut_lanes=1), dict(chunks=1, grabcut_lanes=4),
                                dict(chunks=2, grabcut_lanes=4)])
def test_pipeline_closed_form_leaves_every_other_output_unchanged(pipe, kw):
    from gcn_grabcut import ClosedFormMatte
    from gcn_grabcut._engine import get_engine
    from gcn_grabcut.synthetic import synthetic_batch
    bgr = torch.as_tensor(synthetic_batch(32, 72, 96, config_id=8)).cuda()
    cf = ClosedFormMatte(radius=2, band=2)
    plain = pipe.segment_batch_device(bgr, **kw)
    soft = pipe.segment_batch_device(bgr, matte=cf, **kw)
    one_chunk = pipe.segment_batch_device(bgr, matte=cf, chunks=1, grabcut_lanes=1)
    torch.cuda.synchronize()
    assert "alpha" not in plain and "rgba_soft" not in plain
    for k in ("binary_mask", "trimap", "overlay", "rgba", "gc_mask"):
        assert torch.equal(plain[k], soft[k]), k
    eng = get_engine("cuda")
    want, want_rgba, _, _ = eng.closed_form_matte(bgr, soft["binary_mask"], *cf.args(), want_rgba=True)
    assert torch.equal(soft["alpha"], want) and torch.equal(soft["rgba_soft"], want_rgba)
    assert torch.equal(soft["alpha"], one_chunk["alpha"]) and torch.equal(soft["rgba_soft"], one_chunk["rgba_soft"])


def test_segment_and_segment_bbox_fill_the_closed_form_matte(pipe):
    from gcn_grabcut import ClosedFormMatte, alpha_matte, closed_form_matte
    img, _ = _synthetic(80, 100, 41)
    r = pipe.segment(img, matte=ClosedFormMatte())
    assert r.alpha.shape == (80, 100) and r.rgba_soft.shape == (80, 100, 4)
    assert np.array_equal(r.alpha, closed_form_matte(img, r.binary_mask))
    assert np.abs(r.rgba_soft[..., 3].astype(np.int64) - np.floor(r.alpha.astype(np.float64) * 255.0 + 0.5)).max() <= 1
    assert np.array_equal(pipe.segment(img, matte=True).alpha, alpha_matte(img, r.binary_mask))
    rb = pipe.segment_bbox(img, (20, 15, 60, 50), matte=ClosedFormMatte(band=2))
    assert np.array_equal(rb.alpha, closed_form_matte(img, rb.binary_mask, band=2))
    res = pipe.segment_batch([img, img[::-1].copy()], matte=ClosedFormMatte())
    assert all(np.array_equal(x.alpha, closed_form_matte(x.image, x.binary_mask)) for x in res)
    with pytest.raises(ValueError):
        pipe.segment(img, matte=ClosedFormMatte(), full_image=np.repeat(np.repeat(img, 2, 0), 2, 1))


def test_inference_cli_writes_the_closed_form_matte(tmp_path):
    from PIL import Image
    from helpers import seeded_state_dict
    from gcn_grabcut.synthetic import synthetic_image
    in_dir = tmp_path / "in"
    in_dir.mkdir()
    for k in range(2):
        Image.fromarray(synthetic_image(72, 96, 600 + k)[:, :, ::-1]).save(in_dir / f"im{k}.png")
    _, sd = seeded_state_dict(64, 3, seed=5)
    torch.save({"model": sd, "epoch": 1}, tmp_path / "ckpt.pt")
    out = tmp_path / "cf"
    r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--input", str(in_dir), "--output", str(out),
                        "--checkpoint", str(tmp_path / "ckpt.pt"), "--superpixels", "100", "--max-size", "0",
                        "--matte-method", "closed-form", "--cf-band", "2", "--save", "mask", "alpha", "cutout"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(p.name for p in out.iterdir()) == sorted(f"im{k}_{s}.png" for k in range(2)
                                                           for s in ("mask", "alpha", "cutout"))
    for k in range(2):
        mask = np.asarray(Image.open(out / f"im{k}_mask.png"))
        alpha = Image.open(out / f"im{k}_alpha.png")
        cut = Image.open(out / f"im{k}_cutout.png")
        assert alpha.mode == "L" and alpha.size == (96, 72) and cut.mode == "RGBA" and cut.size == (96, 72)
        a = np.asarray(alpha).astype(np.int64)
        assert np.abs(np.asarray(cut)[..., 3].astype(np.int64) - a).max() <= 1
        far = ~edge_band(mask > 0, 2)
        assert np.array_equal(a[far], (mask[far] > 0).astype(np.int64) * 255)
