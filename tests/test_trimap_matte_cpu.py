"""Trimap matte without a GPU: the float64 restatement (tests/trimap_matte_ref.py) against a direct solve on the dense
matting Laplacian, its identity with the mask-band restatement where the two describe one system, the bound and the
quality ratios the GPU test holds the device to, and the host-side checks of the public call, the engine and the command
lines."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import closed_form_ref as cf
import trimap_matte_ref as tm
from matte_ref import soft_disk_scene

ROOT = Path(__file__).resolve().parent.parent

# What the GPU test (test_trimap_matte_gpu.py) holds the device to, settled on the restatement (tools/trimap_matte_study.py).
R, EPS, MAX_ITER, TOL = 1, 1e-5, 2000, 1e-4
TAU_MEASURED = 0.0375      # max |pcg(tol 1e-4) - pcg(tol 1e-12)| over strands 0-2 and disk0, k in 1, 2, 3, 10, r in 1, 2, both starts
TAU = 2.0 * TAU_MEASURED   # 0.075: the device sums in another order and may stop an iteration earlier or later
RATIO_BAND = {0: 0.557, 1: 0.498, 2: 0.556}     # strands seed -> SAD_U(trimap solve, k = 2) / SAD_U(mask-band matte), restatement
RATIO_MASK = {0: 0.163, 1: 0.154, 2: 0.158}     # ... / SAD_U(hard mask)
QUALITY_SLACK = 0.1        # the device's band ratio may exceed the restatement's by this much
MASK_RATIO_MAX = 0.5


def _noise(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3)).astype(np.uint8), rng


def _ragged(h, w, seed, no_fg=False, border=False):
    """A trimap with a ragged unknown region around a blob; no_fg: the blob is unknown too; border: U reaches the frame."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.hypot(yy - h / 2.0, xx - w / 2.0) + rng.uniform(-1.2, 1.2, (h, w))
    t = np.zeros((h, w), np.uint8)
    t[d < min(h, w) / 2.6] = 128
    t[d < min(h, w) / 5.0] = 128 if no_fg else 255
    t[rng.random((h, w)) < 0.06] = 77                               # stray unknown bytes of another value
    if border:
        t[0, :] = 128
        t[:, w - 1] = 1
        t[h - 1, 2:5] = 254
    return t


TINY = [("ragged", 12, 14, 1, {}), ("ragged_r2", 14, 13, 2, {}), ("no_fg", 11, 12, 1, dict(no_fg=True)),
        ("no_fg_r2", 13, 13, 2, dict(no_fg=True)), ("border", 12, 13, 1, dict(border=True)),
        ("border_r2", 14, 14, 2, dict(border=True))]


@pytest.mark.parametrize("name,h,w,r,kw", TINY)
@pytest.mark.parametrize("start", ["half", "alpha0"])
def test_pcg_matches_a_direct_solve(name, h, w, r, kw, start):
    img, rng = _noise(h, w, 3 * h + w)
    t = _ragged(h, w, h * w, **kw)
    F, G, U = tm.regions(t)
    assert U.any() and not U.all() and G.any() and F.any() != bool(kw.get("no_fg"))
    if kw.get("border"):
        assert U[0].all() and U[:, -1].all()
    a0 = None if start == "half" else rng.uniform(-0.5, 1.5, (h, w))
    want = tm.direct_solve(img, t, r, 1e-5, a0)
    got, it, rel = tm.pcg(img, t, r, 1e-5, 20000, 1e-12, a0)
    assert rel <= 1e-12 and it > 0
    assert np.abs(got - want).max() <= 1e-9, (name, np.abs(got - want).max())
    assert np.array_equal(got[F], np.ones(F.sum())) and np.array_equal(got[G], np.zeros(G.sum()))
    if kw.get("no_fg"):
        assert np.abs(got).max() <= 1e-9                            # nothing is foreground: CG goes to 0


def test_regions_follow_the_benchmark_convention():
    t = np.array([[0, 1, 127, 128, 254, 255]], np.uint8)
    F, G, U = tm.regions(t)
    assert F.tolist() == [[False] * 5 + [True]] and G.tolist() == [[True] + [False] * 5]
    assert U.tolist() == [[False, True, True, True, True, False]]
    x = tm.start_image(t, np.array([[9.0, -3.0, 0.25, 7.0, 0.75, -9.0]]))
    assert x.tolist() == [[0.0, 0.0, 0.25, 1.0, 0.75, 1.0]]
    assert tm.start_image(t).tolist() == [[0.0, 0.5, 0.5, 0.5, 0.5, 1.0]]


def test_trivial_trimaps_return_the_start():
    img, rng = _noise(10, 12, 5)
    a0 = rng.uniform(-1.0, 2.0, (10, 12))
    for value in (0, 255, 128):
        t = np.full((10, 12), value, np.uint8)
        for start in (None, a0):
            x, it, rel = tm.pcg(img, t, 1, 1e-5, 100, 1e-4, start)
            assert it == 0 and rel == 0.0 and np.array_equal(x, tm.start_image(t, start))
    t = np.zeros((10, 12), np.uint8)
    t[3:6, 4:8] = 128                                               # no foreground, start 0: r_0 = 0, nothing to do
    x, it, rel = tm.pcg(img, t, 1, 1e-5, 100, 1e-4, np.zeros((10, 12)))
    assert it == 0 and rel == 0.0 and not x.any()


@pytest.mark.parametrize("scene", ["disk0", "strands0"])
@pytest.mark.parametrize("band,r", [(1, 1), (3, 1), (2, 2)])
def test_the_two_front_ends_describe_one_system(scene, band, r):
    img, _, mask = soft_disk_scene(120, 160, 40.0, 3.0, 0) if scene == "disk0" else cf.strand_scene(120, 160, seed=0)
    t = tm.trimap_from_mask(mask, band)
    assert np.array_equal(tm.regions(t)[2], cf.unknown_band(mask, band))
    want, it_w, rel_w = cf.pcg(img, mask, r, 1e-5, band, 500, 1e-4)
    got, it_g, rel_g = tm.pcg(img, t, r, 1e-5, 500, 1e-4, alpha0=mask)
    assert it_g == it_w and rel_g == rel_w and np.array_equal(got, want)
    a, b = tm.residual_norms(img, t, got, r, 1e-5, alpha0=mask), cf.residual_norms(img, mask, want, r, 1e-5, band)
    assert a == b


def test_trimap_from_alpha_dilates_the_fractional_pixels():
    a = np.zeros((9, 11))
    a[:, 6:] = 1.0
    a[4, 5] = 0.4
    a[0, 0] = 0.7
    t = tm.trimap_from_alpha(a, 2)
    want = np.where(a >= 0.5, 255, 0)
    want[2:7, 3:8] = 128
    want[0:3, 0:3] = 128
    assert np.array_equal(t, want)
    assert np.array_equal(tm.trimap_from_alpha(a, 0) == 128, (a > 0) & (a < 1))


def test_residual_of_the_box_form_is_the_recurrence_residual():
    img, at, mask = cf.strand_scene(120, 160, seed=1)
    t = tm.trimap_from_alpha(at, 2)
    x, it, rel = tm.pcg(img, t, 1, 1e-5, 500, 1e-6)
    res, res0 = tm.residual_norms(img, t, x, 1, 1e-5)
    assert rel <= 1e-6 and abs(res / res0 - rel) <= 0.1 * rel


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_recorded_quality_ratios_are_the_restatements(seed):
    # the figures the GPU quality test compares the device with, recomputed
    img, at, mask = cf.strand_scene(120, 160, seed=seed)
    t = tm.trimap_from_alpha(at, 2)
    U = tm.regions(t)[2]
    x, _, rel = tm.pcg(img, t, R, EPS, MAX_ITER, TOL)
    band, _, _ = cf.pcg(img, mask, 1, 1e-5, 1, 500, 1e-4)
    s = tm.region_sad(np.clip(x, 0, 1), at, U)
    assert rel <= TOL
    assert abs(s / tm.region_sad(np.clip(band, 0, 1), at, U) - RATIO_BAND[seed]) <= 1e-3
    assert abs(s / tm.region_sad(mask, at, U) - RATIO_MASK[seed]) <= 1e-3
    assert RATIO_BAND[seed] + QUALITY_SLACK < 1.0 and RATIO_MASK[seed] < MASK_RATIO_MAX


@pytest.mark.parametrize("k,r,start", [(3, 1, "half"), (10, 1, "mask"), (10, 2, "mask")])
def test_default_tol_is_within_half_tau_of_the_exact_solution(k, r, start):
    # the cases of tools/trimap_matte_study.py --tau that came closest to TAU_MEASURED (0.0268, 0.0375, 0.0204)
    seed = 0 if k == 3 else 1
    img, at, mask = cf.strand_scene(120, 160, seed=seed)
    t = tm.trimap_from_alpha(at, k)
    a0 = None if start == "half" else mask.astype(np.float32)
    a, _, _ = tm.pcg(img, t, r, EPS, MAX_ITER, TOL, a0)
    b, _, rel = tm.pcg(img, t, r, EPS, 50000, 1e-12, a0)
    assert rel <= 1e-12 and np.abs(a - b).max() <= TAU_MEASURED + 5e-5


# ---------------------------------------------------------------- host side, before any device call
def _no_device(monkeypatch):
    from gcn_grabcut import _engine

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_engine, "get_engine", boom)


def test_public_names():
    import gcn_grabcut
    import src.gcn_grabcut as shim
    from gcn_grabcut import pipeline as P
    import inspect
    assert "trimap_matte" in gcn_grabcut.__all__ and hasattr(gcn_grabcut, "trimap_matte") and hasattr(shim, "trimap_matte")
    sig = inspect.signature(gcn_grabcut.trimap_matte)
    assert list(sig.parameters) == ["image", "trimap", "radius", "eps", "max_iter", "tol", "alpha0", "return_info", "device"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["radius"], d["eps"], d["max_iter"], d["tol"]) == (P.CF_RADIUS, P.CF_EPS, P.CF_MAX_ITER, P.CF_TOL)
    assert d["alpha0"] is None and d["return_info"] is False


@pytest.mark.parametrize("what", ["shape", "ndim", "dtype_float", "dtype_bool", "dtype_i32", "a0_shape", "a0_int", "a0_nan",
                                  "a0_inf", "image_dtype", "image_shape", "small"])
def test_trimap_matte_refuses_bad_inputs_on_the_host(monkeypatch, what):
    from gcn_grabcut import trimap_matte
    _no_device(monkeypatch)
    img, rng = _noise(12, 14, 0)
    t = _ragged(12, 14, 1)
    kw = {}
    if what == "shape":
        t = t[:, :7]
    elif what == "ndim":
        t = t[None]
    elif what == "dtype_float":
        t = t.astype(np.float32)
    elif what == "dtype_bool":
        t = t > 0
    elif what == "dtype_i32":
        t = t.astype(np.int32)
    elif what == "a0_shape":
        kw["alpha0"] = np.zeros((12, 13))
    elif what == "a0_int":
        kw["alpha0"] = np.zeros((12, 14), np.uint8)
    elif what in ("a0_nan", "a0_inf"):
        a0 = np.full((12, 14), 0.5, np.float32)
        a0[3, 4] = np.nan if what == "a0_nan" else np.inf
        kw["alpha0"] = a0
    elif what == "image_dtype":
        img = img.astype(np.float32)
    elif what == "image_shape":
        img = img[..., 0]
    elif what == "small":
        img, t, kw = img[:2], t[:2], {}
    with pytest.raises(ValueError):
        trimap_matte(img, t, **kw)


@pytest.mark.parametrize("args", [(0, 1e-5, 10, 1e-4), (9, 1e-5, 10, 1e-4), (1.5, 1e-5, 10, 1e-4), (1, 0.0, 10, 1e-4),
                                  (1, 2.0, 10, 1e-4), (1, float("nan"), 10, 1e-4), (1, 1e-5, 0, 1e-4),
                                  (1, 1e-5, 100001, 1e-4), (1, 1e-5, 10, 0.0), (1, 1e-5, 10, 1.0),
                                  (1, 1e-5, 10, float("inf"))])
def test_host_refuses_out_of_range_arguments(monkeypatch, args):
    import torch
    from gcn_grabcut import trimap_matte
    from gcn_grabcut._engine import Engine
    _no_device(monkeypatch)
    img, _ = _noise(20, 20, 0)
    t = _ragged(20, 20, 2)
    with pytest.raises(ValueError):
        trimap_matte(img, t, *args)
    with pytest.raises(ValueError):
        _dead_engine().trimap_matte(torch.as_tensor(img[None]), torch.as_tensor(t[None]), *args)


def _dead_engine():
    """An Engine whose every library call fails the test: the checks must come first."""
    from gcn_grabcut._engine import Engine
    eng = Engine.__new__(Engine)

    class NoContext:
        def call(self, *a, **k):
            raise AssertionError("a device call was made")
    eng.ctx = NoContext()
    eng.empty = NoContext().call
    return eng


@pytest.mark.parametrize("what", ["shape", "dtype", "a0_shape", "a0_dtype", "small"])
def test_engine_refuses_bad_tensors_before_any_call(what):
    import torch
    img, _ = _noise(12, 14, 0)
    bgr, t = torch.as_tensor(img[None]), torch.as_tensor(_ragged(12, 14, 1)[None])
    a0 = None
    r = 1
    if what == "shape":
        t = t[:, :, :7]
    elif what == "dtype":
        t = t.to(torch.int32)
    elif what == "a0_shape":
        a0 = torch.zeros(1, 12, 13)
    elif what == "a0_dtype":
        a0 = torch.zeros(1, 12, 14, dtype=torch.float64)
    elif what == "small":
        r = 6
    with pytest.raises(ValueError):
        _dead_engine().trimap_matte(bgr, t, r, 1e-5, 10, 1e-4, alpha0=a0)


def test_ctypes_row_matches_the_header():
    import re
    from gcn_grabcut import _native
    header = (ROOT / "include" / "ggc.h").read_text()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bggc_trimap_matte\s*\(([^;]*?)\)\s*;", body, flags=re.S)
    params = [p.strip() for p in m.group(1).split(",")]
    row = _native.SIGNATURES["ggc_trimap_matte"]
    assert len(params) == len(row) == 17
    import ctypes
    for p, c in zip(params, row):
        want = ctypes.c_void_p if "*" in p or "ggc_stream" in p else (ctypes.c_float if p.startswith("float") else ctypes.c_int)
        assert c is want, (p, c)
    assert int(re.search(r"#define GGC_VERSION (\d+)", header).group(1)) >= 401


# ---------------------------------------------------------------- command lines
def _run(script, *argv):
    return subprocess.run([sys.executable, str(ROOT / script), *argv], capture_output=True, text=True, timeout=120)


def _write(path, a):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(a).save(path)


def test_matte_cli_parser():
    sys.path.insert(0, str(ROOT))
    import inference
    import matte
    p = matte.build_parser()
    d = p.parse_args(["--image", "x.png", "--trimap", "t.png"])
    ref = inference.build_parser().parse_args(["--image", "x.png"])
    assert (d.cf_radius, d.cf_eps, d.cf_iters, d.cf_tol) == (ref.cf_radius, ref.cf_eps, ref.cf_iters, ref.cf_tol)
    assert d.save == ["alpha"] and not d.decontaminate and d.output == ref.output
    a = p.parse_args(["--input", "d", "--trimaps", "t", "--save", "alpha", "cutout", "--decontaminate", "--cf-radius", "2",
                      "--cf-eps", "1e-6", "--cf-iters", "50", "--cf-tol", "1e-5"])
    assert (a.cf_radius, a.cf_eps, a.cf_iters, a.cf_tol) == (2, 1e-6, 50, 1e-5) and a.decontaminate
    assert not hasattr(a, "cf_band") and not hasattr(a, "checkpoint")
    for bad in (["--image", "x.png", "--input", "d"], ["--trimap", "t.png"], ["--image", "x.png", "--save", "mask"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_matte_cli_refuses_misuse_without_a_traceback(tmp_path):
    img, _ = _noise(12, 14, 3)
    t = _ragged(12, 14, 1)
    _write(tmp_path / "in" / "x.png", img)
    _write(tmp_path / "tri" / "x.png", t)
    _write(tmp_path / "tri2" / "y.png", t)
    _write(tmp_path / "small" / "x.png", t[:, :5].copy())
    (tmp_path / "empty").mkdir()
    x, tri, ind = str(tmp_path / "in" / "x.png"), str(tmp_path / "tri" / "x.png"), str(tmp_path / "in")
    out = ["--output", str(tmp_path / "out")]
    cases = [(["--image", x], "--trimap"),
             (["--image", x, "--trimaps", str(tmp_path / "tri")], "--trimap"),
             (["--input", ind], "--trimaps"),
             (["--input", ind, "--trimap", tri], "--trimaps"),
             (["--image", x, "--trimap", tri, "--decontaminate"], "cutout"),
             (["--image", x, "--trimap", tri, "--cf-radius", "9"], "radius"),
             (["--image", x, "--trimap", tri, "--cf-tol", "2"], "tol"),
             (["--image", x, "--trimap", tri, "--cf-iters", "0"], "max_iter"),
             (["--image", x, "--trimap", tri, "--cf-radius", "6"], "2r+1"),
             (["--image", x, "--trimap", str(tmp_path / "small" / "x.png")], "is 5x12 but"),
             (["--image", x, "--trimap", str(tmp_path / "nothing.png")], "does not exist"),
             (["--input", ind, "--trimaps", str(tmp_path / "tri2")], "no trimap"),
             (["--input", ind, "--trimaps", str(tmp_path / "missing")], "does not exist"),
             (["--input", str(tmp_path / "empty"), "--trimaps", str(tmp_path / "tri")], "no image files")]
    for argv, word in cases:
        r = _run("matte.py", *argv, *out)
        assert r.returncode != 0 and word in r.stderr and "Traceback" not in r.stderr, (argv, r.returncode, r.stderr)
    assert not (tmp_path / "out").exists()


def test_evaluate_matte_cli_refuses_trimap_misuse_without_a_traceback(tmp_path):
    img, _ = _noise(12, 14, 3)
    t = _ragged(12, 14, 1)
    _write(tmp_path / "gt" / "x.png", t)
    _write(tmp_path / "in" / "x.png", img)
    _write(tmp_path / "tri" / "x.png", t)
    _write(tmp_path / "tri2" / "y.png", t)
    gt, ind, tri = str(tmp_path / "gt"), str(tmp_path / "in"), str(tmp_path / "tri")
    cases = [(["--alphas", gt, "--images", ind, "--method", "trimap"], "--trimaps"),
             (["--alphas", gt, "--images", ind, "--trimaps", tri, "--masks", tri, "--method", "trimap"], "drop --masks"),
             (["--alphas", gt, "--trimaps", tri, "--masks", tri, "--method", "trimap"], "drop --masks"),
             (["--alphas", gt, "--trimaps", tri, "--method", "trimap"], "either --pred"),
             (["--alphas", gt, "--images", ind, "--trimaps", tri, "--method", "trimap", "--cf-radius", "9"], "radius"),
             (["--alphas", gt, "--images", ind, "--trimaps", tri, "--method", "trimap", "--cf-tol", "2"], "tol"),
             (["--alphas", gt, "--images", ind, "--trimaps", tri, "--method", "trimap", "--cf-radius", "6"], "2r+1"),
             (["--alphas", gt, "--images", ind, "--trimaps", str(tmp_path / "tri2"), "--method", "trimap"], "no trimap"),
             (["--alphas", gt, "--images", ind, "--trimaps", tri], "go together")]        # the default method still wants masks
    for argv, word in cases:
        r = _run("evaluate_matte.py", *argv)
        assert r.returncode != 0 and word in r.stderr and "Traceback" not in r.stderr, (argv, r.returncode, r.stderr)
