"""Closed-form alpha matte without a GPU: the float64 restatement (tests/closed_form_ref.py) against the matting
Laplacian assembled from its definition and against a direct solve, the quality margin the GPU test holds the device
to, and the host-side argument checks of the engine, the pipeline and the command line."""
import numpy as np
import pytest

from closed_form_ref import (Laplacian, band_sad, dense_laplacian, direct_solve, laplacian_apply, laplacian_diagonal,
                             pcg, strand_scene, unknown_band)
from matte_ref import alpha_matte_ref, edge_band, soft_disk_scene

DEFAULTS = dict(r=1, eps=1e-5, band=1, max_iter=500, tol=1e-4)      # pipeline.CF_* (checked below)
QUALITY = 0.8          # closed-form band SAD <= QUALITY * the guided matte's (measured: 0.43, 0.65, 0.64 at the defaults)
TAU = 0.05             # device alpha at the default tol vs the restatement at 1e-12 (measured here: below 0.013)


def _noise(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3)).astype(np.uint8), (rng.random((h, w)) < 0.5).astype(np.uint8)


def _scenes():
    for seed in (0, 1):
        yield f"disk{seed}", soft_disk_scene(120, 160, 40.0, 3.0, seed)
    yield "strands0", strand_scene(120, 160, seed=0)


@pytest.mark.parametrize("h,w,r", [(9, 11, 1), (14, 13, 2)])
@pytest.mark.parametrize("eps", [1e-7, 1e-5, 1e-2])
def test_box_form_matches_the_definition(h, w, r, eps):
    img, _ = _noise(h, w, 3 * h + w)
    L = dense_laplacian(img, r, eps)
    rng = np.random.default_rng(h * w)
    for _ in range(3):
        p = rng.standard_normal((h, w))
        want = (L @ p.reshape(-1)).reshape(h, w)
        assert np.abs(laplacian_apply(img, p, r, eps) - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(L - L.T).max() <= 1e-12 * np.abs(L).max()
    assert np.abs(L.sum(1)).max() <= 1e-10
    assert np.linalg.eigvalsh(L).min() >= -1e-10
    assert np.abs(laplacian_diagonal(img, r, eps).reshape(-1) - np.diag(L)).max() <= 1e-10 * np.abs(np.diag(L)).max()


def test_null_space_is_the_constants():
    img, _ = _noise(9, 10, 4)
    L = dense_laplacian(img, 1, 1e-5)
    ev = np.linalg.eigvalsh(L)
    assert abs(ev[0]) <= 1e-10 and ev[1] > 1e-9


@pytest.mark.parametrize("h,w,r,band", [(12, 14, 1, 1), (15, 13, 2, 2), (16, 16, 1, 3)])
def test_pcg_matches_a_direct_solve(h, w, r, band):
    img, _ = _noise(h, w, h + 7 * w)
    yy, xx = np.mgrid[0:h, 0:w]
    mask = ((yy - h / 2) ** 2 + (xx - w / 2) ** 2 < (min(h, w) / 3) ** 2).astype(np.uint8)
    U = unknown_band(mask, band)
    assert U.any() and not U.all()
    want = direct_solve(img, mask, r, 1e-5, band)
    got, it, rel = pcg(img, mask, r, 1e-5, band, 10000, 1e-12)
    assert rel <= 1e-12 and np.abs(got - want).max() <= 1e-8
    assert np.array_equal(got[~U], mask[~U].astype(np.float64))


def test_trivial_images_keep_the_mask():
    img, _ = _noise(10, 12, 5)
    for m in (np.zeros((10, 12), np.uint8), np.ones((10, 12), np.uint8)):
        x, it, rel = pcg(img, m, 1, 1e-5, 2, 100, 1e-4)
        assert it == 0 and np.array_equal(x, m.astype(np.float64))
    m = np.zeros((10, 12), np.uint8)
    m[4:6, 5:7] = 1
    x, it, _ = pcg(img, m, 1, 1e-5, 64, 100, 1e-4)                  # every pixel in U: nothing anchors it
    assert unknown_band(m, 64).all() and it == 0 and np.array_equal(x, m.astype(np.float64))


@pytest.mark.parametrize("name,scene", list(_scenes()))
def test_closed_form_beats_the_guided_matte_on_soft_edges(name, scene):
    # the margin the GPU test holds the device to, settled here at the defaults (tools/closed_form_study.py)
    img, alpha_true, mask = scene
    region = edge_band(mask, 8)
    d = DEFAULTS
    x, it, rel = pcg(img, mask, d["r"], d["eps"], d["band"], d["max_iter"], d["tol"])
    assert rel <= d["tol"]
    guided = band_sad(alpha_matte_ref(img, mask, 4, 1e-4), alpha_true, region)
    assert band_sad(np.clip(x, 0.0, 1.0), alpha_true, region) <= QUALITY * guided, name


def test_strand_scene_has_strands_the_mask_misses():
    img, alpha_true, mask = strand_scene(120, 160, seed=0)
    thin = (alpha_true > 0.3) & (alpha_true < 0.7)
    assert thin.sum() > 100 and np.abs(mask - alpha_true)[thin].mean() > 0.35


@pytest.mark.parametrize("r", [1, 2, 4])
def test_default_tol_is_within_tau_of_the_exact_solution(r):
    from gcn_grabcut.synthetic import synthetic_image
    img, gt = synthetic_image(96, 128, 3, return_mask=True)
    cases = [s for _, s in _scenes()] + [(img, None, gt)]
    for img, _, m in cases:
        a, _, _ = pcg(img, m, r, DEFAULTS["eps"], DEFAULTS["band"], DEFAULTS["max_iter"], DEFAULTS["tol"])
        b, _, rel = pcg(img, m, r, DEFAULTS["eps"], DEFAULTS["band"], 20000, 1e-12)
        assert rel <= 1e-12 and np.abs(np.clip(a, 0, 1) - np.clip(b, 0, 1)).max() <= TAU / 2


def test_residual_of_the_box_form_is_the_recurrence_residual():
    img, alpha_true, mask = soft_disk_scene(60, 80, 20.0, 3.0, 2)
    x, it, rel = pcg(img, mask, 2, 1e-5, 2, 500, 1e-6)
    U = unknown_band(mask, 2)
    L = Laplacian(img, 2, 1e-5)
    true_rel = np.linalg.norm(L.apply(x)[U]) / np.linalg.norm(L.apply(mask.astype(np.float64))[U])
    assert abs(true_rel - rel) <= 0.1 * rel


# ---------------------------------------------------------------- host side, before any device call
def test_defaults_are_the_recorded_choice():
    from gcn_grabcut import ClosedFormMatte
    from gcn_grabcut import pipeline as P
    c = ClosedFormMatte()
    assert c.args() == (DEFAULTS["r"], DEFAULTS["eps"], DEFAULTS["band"], DEFAULTS["max_iter"], DEFAULTS["tol"])
    assert (P.CF_RADIUS, P.CF_EPS, P.CF_BAND, P.CF_MAX_ITER, P.CF_TOL) == c.args()
    with pytest.raises(Exception):
        c.radius = 2                                             # frozen


@pytest.mark.parametrize("args", [(0, 1e-5, 1, 10, 1e-4), (9, 1e-5, 1, 10, 1e-4), (1.5, 1e-5, 1, 10, 1e-4),
                                  (1, 0.0, 1, 10, 1e-4), (1, 2.0, 1, 10, 1e-4), (1, float("nan"), 1, 10, 1e-4),
                                  (1, 1e-5, -1, 10, 1e-4), (1, 1e-5, 65, 10, 1e-4), (1, 1e-5, 1, 0, 1e-4),
                                  (1, 1e-5, 1, 100001, 1e-4), (1, 1e-5, 1, 10, 0.0), (1, 1e-5, 1, 10, 1.0),
                                  (1, 1e-5, 1, 10, float("inf"))])
def test_host_refuses_bad_closed_form_arguments(args):
    from gcn_grabcut import closed_form_matte
    from gcn_grabcut._engine import check_closed_form_args
    with pytest.raises(ValueError):
        check_closed_form_args(*args)
    img, mask = _noise(20, 20, 0)
    with pytest.raises(ValueError):
        closed_form_matte(img, mask, *args)


@pytest.mark.parametrize("h,w,r", [(2, 10, 1), (10, 2, 1), (4, 30, 2), (30, 16, 8)])
def test_host_refuses_images_smaller_than_a_window(h, w, r):
    from gcn_grabcut import closed_form_matte
    img, mask = _noise(h, w, 1)
    with pytest.raises(ValueError, match="2r\\+1"):
        closed_form_matte(img, mask, radius=r)


@pytest.mark.parametrize("bad", [2, 255])
def test_public_closed_form_matte_refuses_non_binary_masks(bad):
    from gcn_grabcut import closed_form_matte
    img, mask = _noise(12, 12, 2)
    mask[3, 3] = bad
    with pytest.raises(ValueError, match="0 or 1"):
        closed_form_matte(img, mask)
    with pytest.raises(ValueError):
        closed_form_matte(img, mask[:, :6])


def test_pipeline_routes_the_closed_form_matte_on_its_own_path():
    from gcn_grabcut import ClosedFormMatte
    from gcn_grabcut.pipeline import _closed_form_args, _matte_args
    assert _matte_args(True, 4, 1e-4) == (4, 1e-4) and _matte_args(False, 0, -1.0) is None
    assert _closed_form_args(True, 50, 50, False) is None and _closed_form_args(False, 50, 50, True) is None
    assert _closed_form_args(ClosedFormMatte(radius=2, band=3), 50, 50, False) == (2, 1e-5, 3, 500, 1e-4)
    with pytest.raises(ValueError, match="full"):
        _closed_form_args(ClosedFormMatte(), 50, 50, True)
    with pytest.raises(ValueError):
        _closed_form_args(ClosedFormMatte(eps=0.0), 50, 50, False)
    with pytest.raises(ValueError):
        _closed_form_args(ClosedFormMatte(radius=4), 8, 50, False)


def test_pipeline_refuses_closed_form_with_full_image_before_any_stage(monkeypatch):
    # no stage may run: the pipeline object is built without a device and every stage entry raises if reached
    from gcn_grabcut import ClosedFormMatte, GCNGrabCutPipeline
    pipe = GCNGrabCutPipeline.__new__(GCNGrabCutPipeline)

    def stage(*a, **k):
        raise AssertionError("a stage ran")

    class NoEngine:
        def __getattr__(self, name):
            return stage

    pipe._eng = NoEngine()
    img, _ = _noise(40, 50, 3)
    for call in (lambda: pipe.segment(img, matte=ClosedFormMatte(), full_image=img),
                 lambda: pipe.segment_bbox(img, (5, 5, 30, 20), matte=ClosedFormMatte(), full_image=img),
                 lambda: pipe.segment_batch([img, img], matte=ClosedFormMatte(), full_images=[img, img])):
        with pytest.raises(ValueError, match="full"):
            call()


def test_cli_offers_the_closed_form_matte():
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import inference
    p = inference.build_parser()
    d = p.parse_args(["--image", "x.png"])
    assert d.matte_method == "guided" and d.matte_radius == 4 and d.matte_eps == 1e-4
    assert (d.cf_radius, d.cf_eps, d.cf_band, d.cf_iters, d.cf_tol) == (1, 1e-5, 1, 500, 1e-4)
    a = p.parse_args(["--image", "x.png", "--save", "alpha", "cutout", "--matte-method", "closed-form", "--cf-radius",
                      "2", "--cf-eps", "1e-6", "--cf-band", "3", "--cf-iters", "50", "--cf-tol", "1e-5"])
    assert a.matte_method == "closed-form" and (a.cf_radius, a.cf_eps, a.cf_band, a.cf_iters, a.cf_tol) == \
        (2, 1e-6, 3, 50, 1e-5)
    with pytest.raises(SystemExit):
        p.parse_args(["--image", "x.png", "--matte-method", "levin"])
    help_text = p.format_help()
    for flag in ("--matte-method", "--cf-radius", "--cf-eps", "--cf-band", "--cf-iters", "--cf-tol"):
        assert flag in help_text


def test_cli_refuses_closed_form_with_full_res(tmp_path):
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(root / "inference.py"), "--image", str(tmp_path / "x.png"), "--full-res",
                        "--matte-method", "closed-form", "--save", "alpha"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "full-res" in r.stderr
