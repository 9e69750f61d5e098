"""ggc_upsample_matte on the MI355X: against the float64 restatement (tests/upsample_ref.py), scale 1 against
ggc_alpha_matte bit for bit, exact far field, batch independence, a photo-sized image, the entry's refusals, the
pipeline's full-resolution outputs and the command line's --full-res."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from matte_ref import soft_disk_scene
from upsample_ref import far_field, mean_coefficients, resize_bgr, upsample_ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _stream():
    from gcn_grabcut import _native
    return _native.current_stream(0)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _call(ctx, bgr, binary, full, r, eps, want=("alpha", "binary", "rgba")):
    """ggc_upsample_matte on (B,H,W,3) / (B,H,W) / (B,H1,W1,3) uint8 arrays -> dict of device tensors."""
    bgr, binary, full = _dev(bgr), _dev(binary), _dev(full)
    b, h, w, _ = bgr.shape
    h1, w1 = full.shape[1:3]
    out = {}
    if "alpha" in want:
        out["alpha"] = torch.empty(b, h1, w1, device="cuda")
    if "binary" in want:
        out["binary"] = torch.empty(b, h1, w1, dtype=torch.uint8, device="cuda")
    if "rgba" in want:
        out["rgba"] = torch.empty(b, h1, w1, 4, dtype=torch.uint8, device="cuda")
    p = lambda k: out[k].data_ptr() if k in out else None                  # noqa: E731
    ctx.call("ggc_upsample_matte", _stream(), b, h, w, bgr.data_ptr(), binary.data_ptr(), h1, w1, full.data_ptr(), r, eps,
             p("alpha"), p("binary"), p("rgba"))
    return out


def _matte(ctx, bgr, binary, r, eps):
    bgr, binary = _dev(bgr), _dev(binary)
    b, h, w, _ = bgr.shape
    alpha = torch.empty(b, h, w, device="cuda")
    rgba = torch.empty(b, h, w, 4, dtype=torch.uint8, device="cuda")
    ctx.call("ggc_alpha_matte", _stream(), b, h, w, bgr.data_ptr(), binary.data_ptr(), r, eps, alpha.data_ptr(),
             rgba.data_ptr())
    return alpha, rgba


def _synthetic(h, w, seed):
    from gcn_grabcut.synthetic import synthetic_image
    return synthetic_image(h, w, seed, return_mask=True)


def _scenes():
    from gcn_grabcut import GrabCut
    out = []
    img, _, mask = soft_disk_scene(97, 131, 30.0, 3.0, 2)
    out.append(("disk97x131", img, mask))
    img, _, mask = soft_disk_scene(60, 80, 22.0, 2.0, 3)
    out.append(("disk60x80", img, mask))
    img, _ = _synthetic(72, 96, 7)
    mask = GrabCut(img).run_with_bbox((15, 10, 60, 50)).astype(np.uint8)
    assert 0 < mask.sum() < mask.size
    out.append(("grabcut72x96", img, mask))
    return out


def _check(got, img, mask, full, r, eps, name):
    ref = upsample_ref(img, mask, full, r, eps)
    a = got["alpha"][0].cpu().numpy().astype(np.float64)
    err = np.abs(a - ref).max()
    assert err <= 2e-5, (name, r, eps, err)
    clear = np.abs(ref - 0.5) > 1e-5
    assert np.array_equal(got["binary"][0].cpu().numpy()[clear], (ref >= 0.5)[clear].astype(np.uint8)), (name, r, eps)
    rgba = got["rgba"][0].cpu().numpy()
    assert np.array_equal(rgba[..., :3], full), name
    assert np.array_equal(rgba[..., 3], np.floor(a * 255.0 + 0.5).astype(np.uint8)), name


@pytest.mark.parametrize("ratio", [1.0, 2.0, 2.5, 3.7])
@pytest.mark.parametrize("r", [1, 4, 8])
@pytest.mark.parametrize("eps", [1e-4, 1e-2])
def test_device_matches_the_restatement(gpu_ctx, ratio, r, eps):
    for name, img, mask in _scenes():
        h1, w1 = int(round(img.shape[0] * ratio)), int(round(img.shape[1] * ratio))
        full = resize_bgr(img, h1, w1)
        got = _call(gpu_ctx, img[None], mask[None], full[None], r, eps)
        _check(got, img, mask, full, r, eps, f"{name}->{h1}x{w1}")


def test_device_matches_the_restatement_on_odd_sizes(gpu_ctx):
    img, _, mask = soft_disk_scene(97, 131, 30.0, 3.0, 5)
    for (h1, w1) in ((300, 401), (97, 132), (98, 131), (211, 131), (101, 1000)):
        full = resize_bgr(img, h1, w1)
        for r, eps in ((1, 1e-2), (4, 1e-4)):
            _check(_call(gpu_ctx, img[None], mask[None], full[None], r, eps), img, mask, full, r, eps, (h1, w1))


def test_tiny_and_degenerate_shapes(gpu_ctx):
    rng = np.random.default_rng(3)
    for (h, w, h1, w1) in ((1, 1, 1, 1), (1, 1, 5, 9), (1, 7, 3, 20), (6, 1, 13, 4), (2, 3, 2, 8)):
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        mask = (rng.random((h, w)) < 0.5).astype(np.uint8)
        full = rng.integers(0, 256, (h1, w1, 3)).astype(np.uint8)
        _check(_call(gpu_ctx, img[None], mask[None], full[None], 2, 1e-3), img, mask, full, 2, 1e-3, (h, w, h1, w1))


@pytest.mark.parametrize("r,eps", [(1, 1e-4), (4, 1e-2), (8, 1e-5)])
def test_scale_one_is_the_matte_bit_for_bit(gpu_ctx, r, eps):
    for name, img, mask in _scenes() + [("noise33x47", *(np.random.default_rng(1).integers(0, 256, (33, 47, 3)).astype(np.uint8),
                                                     (np.random.default_rng(2).random((33, 47)) < 0.5).astype(np.uint8)))]:
        got = _call(gpu_ctx, img[None], mask[None], img[None], r, eps)
        alpha, rgba = _matte(gpu_ctx, img[None], mask[None], r, eps)
        assert torch.equal(got["alpha"], alpha), name
        assert torch.equal(got["rgba"], rgba), name
        a = alpha.cpu().numpy()
        clear = np.abs(a - 0.5) > 1e-6                     # the mask is taken on the double, alpha is its float
        assert np.array_equal(got["binary"].cpu().numpy()[clear], (a >= 0.5)[clear].astype(np.uint8)), name


@pytest.mark.parametrize("r", [1, 3, 8])
def test_far_field_is_exactly_the_mask(gpu_ctx, r):
    from gcn_grabcut.pipeline import nearest_upsample
    checked = 0
    for seed in (0, 1, 2):
        img, gt = _synthetic(90, 120, 50 + seed)
        for (h1, w1) in ((180, 240), (333, 444)):
            full = resize_bgr(img, h1, w1)
            got = _call(gpu_ctx, img[None], gt[None], full[None], r, 1e-5)
            far = far_field(gt, r, h1, w1)
            near = nearest_upsample(gt, h1, w1)
            assert np.array_equal(got["alpha"][0].cpu().numpy()[far], near[far].astype(np.float32))
            assert np.array_equal(got["binary"][0].cpu().numpy()[far], near[far])
            checked += int(far.sum())
    assert checked > 0


def test_batch_equals_single_image_calls_bit_for_bit(gpu_ctx):
    rng = np.random.default_rng(12)
    imgs, masks = [], []
    for k in range(8):
        if k % 2:
            img, m = _synthetic(50, 64, 200 + k)
        else:
            img, m = rng.integers(0, 256, (50, 64, 3)).astype(np.uint8), (rng.random((50, 64)) < 0.4).astype(np.uint8)
        imgs.append(img)
        masks.append(m)
    imgs, masks = np.stack(imgs), np.stack(masks)
    for (h1, w1) in ((125, 160), (131, 171)):
        fulls = np.stack([resize_bgr(im, h1, w1) for im in imgs])
        for r, eps in ((4, 1e-4), (9, 1e-5)):
            batch = _call(gpu_ctx, imgs, masks, fulls, r, eps)
            again = _call(gpu_ctx, imgs, masks, fulls, r, eps)
            for k in batch:
                assert torch.equal(batch[k], again[k]), k
            for i in range(len(imgs)):
                one = _call(gpu_ctx, imgs[i:i + 1], masks[i:i + 1], fulls[i:i + 1], r, eps)
                for k in batch:
                    assert torch.equal(one[k][0], batch[k][i]), (k, i)
            for want in (("alpha",), ("binary",), ("rgba",)):
                part = _call(gpu_ctx, imgs, masks, fulls, r, eps, want)
                assert torch.equal(part[want[0]], batch[want[0]]), want


def test_photo_size(gpu_ctx):
    img, _, mask = soft_disk_scene(600, 800, 200.0, 4.0, 9)
    full = resize_bgr(img, 3000, 4000)
    r, eps = 4, 1e-4
    got = _call(gpu_ctx, img[None], mask[None], full[None], r, eps)
    c = mean_coefficients(img, mask, r, eps)
    rows = np.random.default_rng(0).choice(3000, 64, replace=False)
    rows = np.concatenate([rows, [0, 1, 2999]])
    from upsample_ref import source_coords
    y0, y1, wy = source_coords(3000, 600)
    a = got["alpha"][0].cpu().numpy()
    binary = got["binary"][0].cpu().numpy()
    rgba = got["rgba"][0].cpu().numpy()
    for y in rows:                                   # one output row: rows y0, y1 of C are all it needs
        ref = _row_ref(c, full, y, y0[y], y1[y], wy[y])
        assert np.abs(a[y] - ref).max() <= 2e-5, y
        clear = np.abs(ref - 0.5) > 1e-5
        assert np.array_equal(binary[y][clear], (ref >= 0.5)[clear].astype(np.uint8)), y
        assert np.array_equal(rgba[y, :, 3], np.floor(a[y].astype(np.float64) * 255.0 + 0.5).astype(np.uint8)), y
    assert np.array_equal(rgba[..., :3], full)


def _row_ref(c, full, y, y0, y1, wy):
    """One output row of upsample_ref from the coefficients (the whole (3000, 4000) restatement is not needed)."""
    from upsample_ref import source_coords
    x0, x1, wx = source_coords(full.shape[1], c.shape[1])
    top = c[y0][x0] + wx[:, None] * (c[y0][x1] - c[y0][x0])
    bot = c[y1][x0] + wx[:, None] * (c[y1][x1] - c[y1][x0])
    cc = top + wy * (bot - top)
    f = full[y].astype(np.float64)
    return np.clip(cc[:, 0] * f[:, 0] + cc[:, 1] * f[:, 1] + cc[:, 2] * f[:, 2] + cc[:, 3], 0.0, 1.0)


# ---------------------------------------------------------------- arguments
@pytest.mark.parametrize("case,code", [("h1", -2), ("w1", -2), ("side", -2), ("b0", -2), ("radius0", -1), ("radius65", -1),
                                       ("eps0", -1), ("epsneg", -1), ("nullbgr", -1), ("nullfull", -1),
                                       ("noout", -1)])
def test_entry_refuses_bad_arguments(gpu_ctx, case, code):
    from gcn_grabcut import _native
    img, mask = _synthetic(16, 20, 1)
    bgr, binary, full = _dev(img[None]), _dev(mask[None]), _dev(resize_bgr(img, 32, 40)[None])
    alpha = torch.empty(1, 32, 40, device="cuda")
    args = dict(b=1, h=16, w=20, bgr=bgr.data_ptr(), binary=binary.data_ptr(), h1=32, w1=40, full=full.data_ptr(), r=4,
                eps=1e-4, alpha=alpha.data_ptr(), mask=None, rgba=None)
    args.update({"h1": dict(h1=15), "w1": dict(w1=19), "side": dict(w1=32769), "b0": dict(b=0), "radius0": dict(r=0),
                 "radius65": dict(r=65), "eps0": dict(eps=0.0), "epsneg": dict(eps=-1e-3), "nullbgr": dict(bgr=None),
                 "nullfull": dict(full=None), "noout": dict(alpha=None)}[case])
    with pytest.raises(_native.GGCError) as e:
        gpu_ctx.call("ggc_upsample_matte", _stream(), *args.values())
    assert e.value.code == code


def test_engine_refuses_bad_arguments_with_value_error(gpu_ctx):
    from gcn_grabcut._engine import get_engine
    eng = get_engine("cuda")
    img, mask = _synthetic(16, 20, 1)
    bgr, binary, full = _dev(img[None]), _dev(mask[None]), _dev(resize_bgr(img, 32, 40)[None])
    for kw in (dict(radius=0), dict(eps=0.0), dict(want_alpha=False, want_binary=False)):
        with pytest.raises(ValueError):
            eng.upsample_matte(bgr, binary, full, **kw)
    with pytest.raises(ValueError):
        eng.upsample_matte(bgr, binary, full[:, :10])
    with pytest.raises(ValueError):
        eng.upsample_matte(bgr, binary[:, :5], full)


def test_public_upsample_mask(gpu_ctx):
    from gcn_grabcut import alpha_matte, upsample_mask
    img, gt = _synthetic(60, 80, 31)
    full = resize_bgr(img, 150, 200)
    alpha, mask = upsample_mask(img, gt.astype(bool), full, 5, 1e-3)
    assert alpha.dtype == np.float32 and alpha.shape == (150, 200) and mask.dtype == np.uint8
    assert np.abs(alpha - upsample_ref(img, gt, full, 5, 1e-3)).max() <= 2e-5
    same, _ = upsample_mask(img, gt, img, 5, 1e-3)
    assert np.array_equal(same, alpha_matte(img, gt, 5, 1e-3))


# ---------------------------------------------------------------- pipeline and command line
@pytest.fixture(scope="module")
def pipe():
    from helpers import seeded_state_dict
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig
    model, _ = seeded_state_dict(64, 3, seed=4)
    return GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=100), device="cuda:0")


@pytest.mark.parametrize("kw", [dict(chunks=1, grabcut_lanes=1), dict(chunks=1, grabcut_lanes=4)])
@pytest.mark.parametrize("matte", [False, True])
def test_pipeline_full_resolution_outputs(pipe, kw, matte):
    from gcn_grabcut._engine import get_engine
    from gcn_grabcut.synthetic import synthetic_batch
    imgs = synthetic_batch(32, 72, 96, config_id=8)
    bgr = _dev(imgs)
    full_bgr = _dev(np.stack([resize_bgr(im, 180, 241) for im in imgs]))
    plain = pipe.segment_batch_device(bgr, matte=matte, matte_radius=3, matte_eps=1e-3, **kw)
    big = pipe.segment_batch_device(bgr, matte=matte, matte_radius=3, matte_eps=1e-3, full_bgr=full_bgr, **kw)
    torch.cuda.synchronize()
    assert "full" not in plain
    for k in ("binary_mask", "trimap", "overlay", "rgba", "gc_mask") + (("alpha", "rgba_soft") if matte else ()):
        assert torch.equal(plain[k], big[k]), k
    f = big["full"]
    assert sorted(f) == sorted(["binary_mask", "overlay", "rgba"] + (["alpha", "rgba_soft"] if matte else []))
    assert f["binary_mask"].shape == (32, 180, 241) and f["overlay"].shape == (32, 180, 241, 3)
    eng = get_engine("cuda")
    alpha, mask, soft = eng.upsample_matte(bgr, big["binary_mask"], full_bgr, 3, 1e-3, want_rgba=True)
    assert torch.equal(f["binary_mask"], mask)
    if matte:
        assert f["alpha"].shape == (32, 180, 241) and torch.equal(f["alpha"], alpha) and torch.equal(f["rgba_soft"], soft)
    overlay, rgba = eng.compose(full_bgr, f["binary_mask"])
    assert torch.equal(f["overlay"], overlay) and torch.equal(f["rgba"], rgba)


def test_chunked_path_equals_one_chunk(pipe):
    from gcn_grabcut.synthetic import synthetic_batch
    imgs = synthetic_batch(32, 72, 96, config_id=9)
    bgr = _dev(imgs)
    full_bgr = _dev(np.stack([resize_bgr(im, 144, 192) for im in imgs]))
    one = pipe.segment_batch_device(bgr, matte=True, full_bgr=full_bgr, chunks=1, grabcut_lanes=4)
    two = pipe.segment_batch_device(bgr, matte=True, full_bgr=full_bgr, chunks=2, grabcut_lanes=4)
    torch.cuda.synchronize()
    for k in one["full"]:
        assert torch.equal(one["full"][k], two["full"][k]), k


def test_segment_batch_segment_and_segment_bbox_fill_full(pipe):
    from gcn_grabcut import upsample_mask
    img, _ = _synthetic(80, 100, 41)
    full = resize_bgr(img, 200, 250)
    r = pipe.segment(img, full_image=full, matte=True)
    assert r.full.binary_mask.shape == (200, 250) and r.full.rgba.shape == (200, 250, 4)
    alpha, mask = upsample_mask(img, r.binary_mask, full)
    assert np.array_equal(r.full.alpha, alpha) and np.array_equal(r.full.binary_mask, mask)
    assert pipe.segment(img).full is None
    assert pipe.segment(img, full_image=full).full.alpha is None
    rb = pipe.segment_bbox(img, (20, 15, 60, 50), full_image=full, matte_radius=3)
    assert np.array_equal(rb.full.binary_mask, upsample_mask(img, rb.binary_mask, full, 3)[1])
    assert rb.full.alpha is None and rb.full.overlay.shape == (200, 250, 3)
    imgs = [img, img[::-1].copy()]
    res = pipe.segment_batch(imgs, full_images=[full, full[::-1].copy()])
    plain = pipe.segment_batch(imgs)
    for x, p in zip(res, plain):
        assert np.array_equal(x.binary_mask, p.binary_mask) and np.array_equal(x.overlay, p.overlay)
        assert x.full.binary_mask.shape == (200, 250)
    with pytest.raises(ValueError):
        pipe.segment_batch(imgs, full_images=[full, full[:, :240].copy()])


def test_inference_cli_full_res(tmp_path):
    from PIL import Image
    from helpers import seeded_state_dict
    from gcn_grabcut import upsample_mask
    sys.path.insert(0, str(ROOT))
    import inference
    in_dir = tmp_path / "in"
    in_dir.mkdir()
    img, _ = _synthetic(300, 400, 600)
    Image.fromarray(img[:, :, ::-1]).save(in_dir / "big.png")
    small, _ = _synthetic(72, 96, 601)
    Image.fromarray(small[:, :, ::-1]).save(in_dir / "small.png")
    _, sd = seeded_state_dict(64, 3, seed=5)
    torch.save({"model": sd, "epoch": 1}, tmp_path / "ckpt.pt")
    saves = ["mask", "overlay", "rgba", "trimap", "alpha", "cutout"]

    def run(out, *extra):
        r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--input", str(in_dir), "--output", str(out),
                            "--checkpoint", str(tmp_path / "ckpt.pt"), "--superpixels", "100", "--max-size", "200",
                            "--save", *saves, *extra], cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]

    run(tmp_path / "work")
    run(tmp_path / "full", "--full-res")
    for s in saves:
        im = Image.open(tmp_path / "full" / f"big_{s}.png")
        assert im.size == (400, 300), s
        assert (tmp_path / "full" / f"small_{s}.png").read_bytes() == (tmp_path / "work" / f"small_{s}.png").read_bytes(), s
    resized = inference.read_bgr(in_dir / "big.png", 200)
    work_mask = (np.asarray(Image.open(tmp_path / "work" / "big_mask.png")) > 0).astype(np.uint8)
    assert work_mask.shape == resized.shape[:2] == (150, 200)
    _, want = upsample_mask(resized, work_mask, img)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "full" / "big_mask.png")), want * 255)
