"""Soft alpha matte (colour guided-filter feathering), without a GPU: the float64 restatement in matte_ref.py against a
per-pixel loop and against the properties the filter must have, plus the host-side argument checks and outputs."""
import numpy as np
import pytest

from matte_ref import (alpha_matte_ref, brute_force_matte, edge_band, grey_guided_filter, matte_coefficients,
                       soft_disk_scene)


def _case(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3)).astype(np.uint8), (rng.random((h, w)) < 0.5).astype(np.uint8)


@pytest.mark.parametrize("h,w,r", [(1, 1, 1), (1, 7, 2), (7, 1, 2), (5, 3, 1), (5, 3, 4), (4, 6, 9), (9, 8, 2)])
@pytest.mark.parametrize("eps", [1e-2, 1e-4, 1e-5])
def test_restatement_matches_a_per_pixel_loop(h, w, r, eps):
    img, mask = _case(h, w, 7 * h + w)
    assert np.abs(alpha_matte_ref(img, mask, r, eps) - brute_force_matte(img, mask, r, eps)).max() < 1e-9


def test_alpha_lies_in_the_unit_interval():
    from gcn_grabcut.synthetic import synthetic_image
    img, gt = synthetic_image(90, 120, 4, return_mask=True)
    for r, eps in ((1, 1e-5), (4, 1e-4), (16, 1e-2)):
        a = alpha_matte_ref(img, gt, r, eps)
        assert a.min() >= 0.0 and a.max() <= 1.0
        assert 0.0 < a[edge_band(gt, 2 * r)].mean() < 1.0


@pytest.mark.parametrize("value", [0, 1])
def test_constant_masks_are_kept_exactly(value):
    img, _ = _case(37, 53, 3)
    mask = np.full((37, 53), value, np.uint8)
    for r in (1, 4, 30):
        assert np.array_equal(alpha_matte_ref(img, mask, r, 1e-4), np.full((37, 53), float(value)))


@pytest.mark.parametrize("r,eps", [(2, 1e-2), (4, 1e-4), (8, 1e-3)])
def test_grey_image_is_the_grey_guide_filter_with_a_third_of_eps(r, eps):
    # B = G = R = g: Sigma = var(g) 11^T, so a = cov / (3 var + eps) 1 and a . I = g cov / (var + eps / 3)
    from gcn_grabcut.synthetic import synthetic_image
    img, gt = synthetic_image(60, 80, 11, return_mask=True)
    grey = img[..., 1]
    want = np.clip(grey_guided_filter(grey / 255.0, gt.astype(np.float64), r, eps / 3.0), 0.0, 1.0)
    got = alpha_matte_ref(np.repeat(grey[..., None], 3, axis=2), gt, r, eps)
    assert np.abs(got - want).max() < 1e-8


def test_far_from_the_edge_alpha_equals_the_mask():
    from gcn_grabcut.synthetic import synthetic_image
    img, gt = synthetic_image(80, 100, 5, return_mask=True)
    for r in (1, 3, 6):
        a = alpha_matte_ref(img, gt, r, 1e-4)
        far = ~edge_band(gt, 2 * r)
        assert far.any() and np.abs(a[far] - gt[far]).max() < 1e-9


def test_coefficients_of_a_constant_window_vanish():
    img, _ = _case(20, 20, 9)
    a, b = matte_coefficients(img, np.ones((20, 20), np.uint8), 3, 1e-4)
    assert np.array_equal(a, np.zeros_like(a)) and np.array_equal(b, np.ones_like(b))


@pytest.mark.parametrize("r", [2, 4, 8])
@pytest.mark.parametrize("eps", [1e-2, 1e-4, 1e-5])
@pytest.mark.parametrize("seed", [0, 1])
def test_matte_recovers_a_known_soft_edge(r, eps, seed):
    # the margin the GPU test holds the device to, settled here: in the 2r band around the edge the matte is at least
    # 20 % closer (SAD) to the true alpha than the hard mask is.  The textures are low-frequency: per-pixel noise of
    # +-50 grey levels inside F and B defeats the local linear model at r = 8 (ratio about 1.3 on this scene).
    img, alpha_true, mask = soft_disk_scene(120, 160, 40.0, 3.0, seed)
    band = edge_band(mask, 2 * r)
    a = alpha_matte_ref(img, mask, r, eps)
    assert np.abs(a - alpha_true)[band].sum() <= 0.8 * np.abs(mask - alpha_true)[band].sum()


def test_restatement_runs_a_full_hd_image():
    import time
    from gcn_grabcut.synthetic import synthetic_image
    img, gt = synthetic_image(1080, 1920, 2, return_mask=True)
    t = time.perf_counter()
    a = alpha_matte_ref(img, gt, 8, 1e-4)
    assert a.shape == (1080, 1920) and time.perf_counter() - t < 60.0


# ---------------------------------------------------------------- host side, before any device call
@pytest.mark.parametrize("radius,eps", [(0, 1e-4), (65, 1e-4), (-1, 1e-4), (4, 0.0), (4, -1e-3), (4, float("nan")),
                                        (4, float("inf")), (4, 1e-13), (2.5, 1e-4)])
def test_host_refuses_bad_matte_arguments(radius, eps):
    from gcn_grabcut import alpha_matte
    from gcn_grabcut._engine import check_matte_args
    with pytest.raises(ValueError):
        check_matte_args(radius, eps)
    img, mask = _case(8, 8, 0)
    with pytest.raises(ValueError):
        alpha_matte(img, mask, radius, eps)


@pytest.mark.parametrize("bad", [2, 255])
def test_public_alpha_matte_refuses_non_binary_masks(bad):
    from gcn_grabcut import alpha_matte
    img, mask = _case(8, 8, 1)
    mask[3, 3] = bad
    with pytest.raises(ValueError, match="0 or 1"):
        alpha_matte(img, mask)
    with pytest.raises(ValueError):
        alpha_matte(img, mask[:, :4])


def test_pipeline_refuses_bad_matte_arguments_before_any_stage():
    from gcn_grabcut.pipeline import _matte_args
    assert _matte_args(False, 0, -1.0) is None            # not asked for: not checked
    assert _matte_args(True, 4, 1e-4) == (4, 1e-4)
    with pytest.raises(ValueError):
        _matte_args(True, 65, 1e-4)


def test_segmentation_result_saves_the_matte_only_when_present(tmp_path):
    from PIL import Image
    from gcn_grabcut import SegmentationResult
    img, mask = _case(6, 9, 2)
    kw = dict(image=img, binary_mask=mask, trimap=mask + 2, segments=np.zeros((6, 9), np.int32), overlay=img,
              rgba=np.zeros((6, 9, 4), np.uint8))
    r = SegmentationResult(**kw)
    assert r.alpha is None and r.rgba_soft is None
    r.save(str(tmp_path / "a"))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a_mask.png", "a_overlay.png", "a_rgba.png",
                                                           "a_trimap_colour.png"]
    alpha = np.linspace(0.0, 1.0, 54, dtype=np.float32).reshape(6, 9)
    soft = np.concatenate([img, np.floor(alpha * 255.0 + 0.5).astype(np.uint8)[..., None]], axis=2)
    SegmentationResult(**kw, alpha=alpha, rgba_soft=soft).save(str(tmp_path / "b"))
    a_png = Image.open(tmp_path / "b_alpha.png")
    c_png = Image.open(tmp_path / "b_cutout.png")
    assert a_png.mode == "L" and np.array_equal(np.asarray(a_png), soft[..., 3])
    assert c_png.mode == "RGBA" and np.array_equal(np.asarray(c_png), soft[..., [2, 1, 0, 3]])


def test_cli_offers_the_matte_outputs():
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import inference
    p = inference.build_parser()
    a = p.parse_args(["--image", "x.png", "--save", "mask", "alpha", "cutout", "--matte-radius", "8", "--matte-eps", "1e-3"])
    assert a.save == ["mask", "alpha", "cutout"] and a.matte_radius == 8 and a.matte_eps == 1e-3
    d = p.parse_args(["--image", "x.png"])
    assert d.save == ["mask", "overlay"] and d.matte_radius == 4 and d.matte_eps == 1e-4
