"""Full-resolution masks and mattes (fast guided filter), without a GPU: the float64 restatement in upsample_ref.py
against a per-pixel loop and against the properties the definition gives, plus the host-side argument checks, the
command-line flag and SegmentationResult.save."""
import sys
from pathlib import Path

import numpy as np
import pytest

from matte_ref import alpha_matte_ref
from upsample_ref import brute_force_upsample, far_field, resize_bgr, source_coords, upsample_ref


def _case(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3)).astype(np.uint8), (rng.random((h, w)) < 0.5).astype(np.uint8)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (4, 1), (3, 4), (5, 6)])
@pytest.mark.parametrize("ratio", [1.0, 2.0, 2.5, 3.7])
@pytest.mark.parametrize("r,eps", [(1, 1e-2), (2, 1e-4)])
def test_restatement_matches_a_per_pixel_loop(h, w, ratio, r, eps):
    img, mask = _case(h, w, 11 * h + w)
    h1, w1 = int(round(h * ratio)), int(round(w * ratio))
    full = np.random.default_rng(h1 + w1).integers(0, 256, (h1, w1, 3)).astype(np.uint8)
    got = upsample_ref(img, mask, full, r, eps)
    assert got.shape == (h1, w1)
    assert np.abs(got - brute_force_upsample(img, mask, full, r, eps)).max() < 1e-9


@pytest.mark.parametrize("h,w,r", [(1, 1, 1), (7, 1, 2), (9, 13, 2), (40, 30, 4)])
def test_scale_one_is_the_matte(h, w, r):
    img, mask = _case(h, w, h * w)
    for eps in (1e-2, 1e-4):
        assert np.abs(upsample_ref(img, mask, img, r, eps) - alpha_matte_ref(img, mask, r, eps)).max() < 1e-12


@pytest.mark.parametrize("n,n1", [(1, 1), (1, 7), (5, 5), (4, 8), (4, 10), (10, 37), (97, 300)])
def test_source_coordinates(n, n1):
    i0, i1, w = source_coords(n1, n)
    assert (0 <= i0).all() and (i0 <= i1).all() and (i1 <= n - 1).all() and (i1 - i0 <= 1).all()
    assert (0.0 <= w).all() and (w < 1.0).all()
    if n == n1:
        assert np.array_equal(i0, np.arange(n)) and not w.any()
    pos = i0 + w                                                 # the clamped half-pixel-centre coordinate
    assert np.allclose(pos, np.clip((np.arange(n1) + 0.5) * n / n1 - 0.5, 0, n - 1))


@pytest.mark.parametrize("value", [0, 1])
def test_constant_masks_are_kept_exactly(value):
    img, _ = _case(23, 31, 3)
    full = resize_bgr(img, 60, 77)
    mask = np.full((23, 31), value, np.uint8)
    for r in (1, 4):
        assert np.array_equal(upsample_ref(img, mask, full, r, 1e-4), np.full((60, 77), float(value)))


def test_far_field_keeps_the_mask():
    from gcn_grabcut.synthetic import synthetic_image
    img, gt = synthetic_image(60, 80, 5, return_mask=True)
    full = resize_bgr(img, 150, 200)
    a = upsample_ref(img, gt, full, 2, 1e-4)
    far = far_field(gt, 2, 150, 200)
    from gcn_grabcut.pipeline import nearest_upsample
    assert far.any() and np.abs(a[far] - nearest_upsample(gt, 150, 200)[far]).max() < 1e-9


def test_nearest_upsample_uses_the_pixel_under_each_centre():
    from gcn_grabcut.pipeline import nearest_upsample
    a = np.arange(12).reshape(3, 4)
    assert np.array_equal(nearest_upsample(a, 3, 4), a)
    assert np.array_equal(nearest_upsample(a, 6, 8), np.repeat(np.repeat(a, 2, 0), 2, 1))
    assert nearest_upsample(np.zeros((3, 4, 3)), 7, 9).shape == (7, 9, 3)


# ---------------------------------------------------------------- host side, before any device call
def _no_device(monkeypatch):
    from gcn_grabcut import _engine

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_engine, "get_engine", boom)


@pytest.mark.parametrize("what", ["shape", "smaller", "nonbinary", "radius", "eps", "full3"])
def test_upsample_mask_refuses_bad_arguments_on_the_host(monkeypatch, what):
    from gcn_grabcut import upsample_mask
    _no_device(monkeypatch)
    img, mask = _case(8, 10, 0)
    full = resize_bgr(img, 16, 20)
    kw = {}
    if what == "shape":
        mask = mask[:, :5]
    elif what == "smaller":
        full = full[:7]
    elif what == "nonbinary":
        mask[2, 2] = 255
    elif what == "radius":
        kw = dict(radius=65)
    elif what == "eps":
        kw = dict(eps=0.0)
    elif what == "full3":
        full = full[..., 0]
    with pytest.raises(ValueError):
        upsample_mask(img, mask, full, **kw)


def test_host_shape_rules():
    from gcn_grabcut._engine import check_upsample_shapes
    check_upsample_shapes((2, 5, 6, 3), (2, 5, 6), (2, 5, 6, 3))
    check_upsample_shapes((2, 5, 6, 3), (2, 5, 6), (2, 32768, 6, 3))
    for bad in [((2, 5, 6, 3), (2, 5, 7), (2, 9, 9, 3)), ((2, 5, 6, 3), (2, 5, 6), (1, 9, 9, 3)),
                ((2, 5, 6, 3), (2, 5, 6), (2, 4, 9, 3)), ((2, 5, 6, 3), (2, 5, 6), (2, 9, 5, 3)),
                ((2, 5, 6, 3), (2, 5, 6), (2, 32769, 9, 3)), ((2, 5, 6, 3), (2, 5, 6), (2, 9, 9, 4))]:
        with pytest.raises(ValueError):
            check_upsample_shapes(*bad)


def test_pipeline_checks_the_full_batch_before_any_stage():
    from gcn_grabcut.pipeline import _full_args
    assert _full_args(None, (2, 5, 6, 3), 0, -1.0) is None               # not asked for: not checked
    full = np.zeros((2, 10, 12, 3), np.uint8)
    assert _full_args(full, (2, 5, 6, 3), 4, 1e-4) == (4, 1e-4)
    with pytest.raises(ValueError):
        _full_args(full, (2, 5, 6, 3), 65, 1e-4)
    with pytest.raises(ValueError):
        _full_args(full[:, :4], (2, 5, 6, 3), 4, 1e-4)
    with pytest.raises(ValueError):
        _full_args(full[:1], (2, 5, 6, 3), 4, 1e-4)


def test_cli_offers_full_res_off_by_default():
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import inference
    p = inference.build_parser()
    assert p.parse_args(["--image", "x.png"]).full_res is False
    assert p.parse_args(["--image", "x.png", "--full-res"]).full_res is True
    assert "--full-res" in p.format_help()


def test_read_bgr_keeps_the_original(tmp_path):
    from PIL import Image
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import inference
    img, _ = _case(30, 50, 4)
    Image.fromarray(img[:, :, ::-1]).save(tmp_path / "a.png")
    small = inference.read_bgr(tmp_path / "a.png", 20)
    small2, orig = inference.read_bgr(tmp_path / "a.png", 20, keep_original=True)
    assert small.shape == (12, 20, 3) and np.array_equal(small, small2) and np.array_equal(orig, img)
    same, orig = inference.read_bgr(tmp_path / "a.png", 100, keep_original=True)
    assert np.array_equal(same, img) and np.array_equal(orig, img)


def test_save_writes_the_full_files_only_when_full_is_set(tmp_path):
    from PIL import Image
    from gcn_grabcut import FullResolution, SegmentationResult
    img, mask = _case(6, 9, 2)
    kw = dict(image=img, binary_mask=mask, trimap=mask + 2, segments=np.zeros((6, 9), np.int32), overlay=img,
              rgba=np.zeros((6, 9, 4), np.uint8))
    SegmentationResult(**kw).save(str(tmp_path / "a"))
    plain = ["a_mask.png", "a_overlay.png", "a_rgba.png", "a_trimap_colour.png"]
    assert sorted(p.name for p in tmp_path.iterdir()) == plain
    big, bmask = _case(12, 18, 3)
    rgba = np.concatenate([big, bmask[..., None] * 255], axis=2)
    SegmentationResult(**kw, full=FullResolution(binary_mask=bmask, overlay=big, rgba=rgba)).save(str(tmp_path / "b"))
    assert sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("b_")) == sorted(
        ["b_mask.png", "b_overlay.png", "b_rgba.png", "b_trimap_colour.png", "b_full_mask.png", "b_full_overlay.png",
         "b_full_rgba.png"])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "b_full_mask.png")), bmask * 255)
    alpha = np.linspace(0.0, 1.0, 12 * 18, dtype=np.float32).reshape(12, 18)
    soft = np.concatenate([big, np.floor(alpha * 255.0 + 0.5).astype(np.uint8)[..., None]], axis=2)
    SegmentationResult(**kw, full=FullResolution(binary_mask=bmask, overlay=big, rgba=rgba, alpha=alpha,
                                                 rgba_soft=soft)).save(str(tmp_path / "c"))
    a_png = Image.open(tmp_path / "c_full_alpha.png")
    c_png = Image.open(tmp_path / "c_full_cutout.png")
    assert a_png.size == (18, 12) and np.array_equal(np.asarray(a_png), soft[..., 3])
    assert c_png.mode == "RGBA" and np.array_equal(np.asarray(c_png), soft[..., [2, 1, 0, 3]])
