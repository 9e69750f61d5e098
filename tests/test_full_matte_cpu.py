"""Full-resolution closed-form matte without a GPU: the float64 restatement (tests/full_matte_ref.py) of the lift against a
per-pixel loop, its identities, the warm stop rule against trimap_matte_ref.pcg, the recorded figures the GPU test
(test_full_matte_gpu.py) holds the device to, and the host-side argument checks of the new public functions."""
import functools
import inspect
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import full_matte_ref as fm
import trimap_matte_ref as tm
from closed_form_ref import strand_scene

ROOT = Path(__file__).resolve().parent.parent

# What the GPU test holds the device to, settled on the restatement (tools/full_matte_study.py).
TAU_MEASURED = 0.0147          # max |pcg_warm(tol 1e-4) - pcg_warm(tol 1e-12)| over fm.WARM_CASES (--tau)
TAU = 2.0 * TAU_MEASURED       # the §5.16 convention: the device may stop an iteration apart from the restatement
RATIO = {0: 0.4483, 1: 0.4808}  # whole-image SAD, full-size solve / upsampled hard mask, 480x640 from 120x160 (--quality)
QUALITY_SLACK = 0.1            # the margin §5.16 gives a device sum order
WARM_ITERS = {0: 198, 1: 211}
COLD_ITERS = {0: 286, 1: 304}


def _random_case(h, w, seed):
    rng = np.random.default_rng(seed)
    t = rng.choice(np.array([0, 255, 128, 37, 254, 1], np.uint8), size=(h, w), p=[0.35, 0.35, 0.1, 0.1, 0.05, 0.05])
    # blocks, so that whole neighbourhoods are known
    t[: h // 2, : w // 2] = 255
    t[h // 2 + 1:, w // 2 + 1:] = 0
    a = rng.uniform(-0.3, 1.3, (h, w)).astype(np.float32)
    a[rng.integers(0, h), rng.integers(0, w)] = np.nan
    return t, a


LIFT_SHAPES = [((7, 9), (7, 9)), ((7, 9), (14, 18)), ((6, 9), (20, 30)), ((7, 9), (28, 36)), ((5, 7), (11, 20)),
               ((9, 6), (10, 23))]


@pytest.mark.parametrize("grow", [0, 1, 5])
@pytest.mark.parametrize("shape,full", LIFT_SHAPES)
def test_lift_equals_the_per_pixel_loop(shape, full, grow):
    t, a = _random_case(*shape, seed=shape[0] * 31 + full[1] + grow)
    got_t, got_a = fm.lift(t, a, full, grow)
    want_t, want_a = fm.brute_force_lift(t, a, full, grow)
    assert got_t.dtype == np.uint8 and got_a.dtype == np.float32 and got_t.shape == full == got_a.shape
    assert np.array_equal(got_t, want_t)
    assert np.array_equal(got_a, want_a)
    assert set(np.unique(got_t)) <= {0, 128, 255}
    assert got_a.min() >= 0.0 and got_a.max() <= 1.0


def test_lift_at_the_same_size_is_the_identity():
    t, a = _random_case(13, 17, 3)
    got_t, got_a = fm.lift(t, a, (13, 17), 0)
    assert np.array_equal(got_t, np.where(t == 255, 255, np.where(t == 0, 0, 128)))
    assert np.array_equal(got_a, np.clip(np.where(np.isnan(a), 0.0, a), 0.0, 1.0).astype(np.float32))


@pytest.mark.parametrize("byte,want", [(255, 255), (0, 0), (128, 128), (7, 128)])
def test_constant_trimap_lifts_to_a_constant(byte, want):
    t = np.full((6, 8), byte, np.uint8)
    for grow in (0, 3):
        got_t, got_a = fm.lift(t, np.full((6, 8), 0.25), (15, 27), grow)
        assert (got_t == want).all()
        assert (got_a == np.float32(0.25)).all()


@pytest.mark.parametrize("shape,full", LIFT_SHAPES)
def test_lifted_known_regions_lie_inside_the_nearest_neighbour_ones(shape, full):
    from gcn_grabcut.pipeline import nearest_upsample
    t, a = _random_case(*shape, seed=5)
    near = nearest_upsample(t, *full)
    for grow in (0, 2):
        got_t, _ = fm.lift(t, a, full, grow)
        assert (near[got_t == 255] == 255).all() and (near[got_t == 0] == 0).all()
    assert (fm.lift(t, a, full, 0)[0] == 255).any() and (fm.lift(t, a, full, 0)[0] == 0).any()


def _small_scene(seed=0):
    img, at, _ = strand_scene(40, 52, radius=13.0, seed=seed)
    return img, tm.trimap_from_alpha(at, 2), at


def test_warm_from_one_half_is_the_cold_solve():
    img, t, _ = _small_scene()
    half = np.full(t.shape, 0.5)
    for max_iter, tol in ((500, 1e-4), (7, 1e-9)):
        a, it, rel = fm.pcg_warm(img, t, 1, 1e-5, max_iter, tol, half)
        b, it_b, rel_b = tm.pcg(img, t, 1, 1e-5, max_iter, tol)
        assert np.array_equal(a, b) and it == it_b and rel == rel_b


def test_warm_stop_rule():
    img, t, _ = _small_scene(1)
    U = tm.regions(t)[2]
    exact = tm.direct_solve(img, t, 1, 1e-5)
    # a start that is already good enough comes back as it is (the start is clamped, so the exact solution, which
    # leaves [0, 1], is good only to rel0)
    res0, ref0 = fm.residual_norms(img, t, tm.start_image(t, exact), 1, 1e-5)
    rel0 = res0 / ref0
    assert 0.0 < rel0 < 0.5
    a, it, rel = fm.pcg_warm(img, t, 1, 1e-5, 500, rel0 * 1.001, exact)
    assert it == 0 and rel == pytest.approx(rel0, rel=1e-9) and np.array_equal(a, tm.start_image(t, exact))
    assert fm.pcg_warm(img, t, 1, 1e-5, 500, rel0 * 0.5, exact)[1] > 0
    # the stop does not move with the start: every start ends under the same absolute residual
    _, ref = fm.residual_norms(img, t, exact, 1, 1e-5)
    rng = np.random.default_rng(0)
    for start in (np.zeros(t.shape), exact + 0.05 * rng.standard_normal(t.shape), np.full(t.shape, 0.5)):
        a, it, rel = fm.pcg_warm(img, t, 1, 1e-5, 500, 1e-4, start)
        res, ref2 = fm.residual_norms(img, t, a, 1, 1e-5)
        assert ref2 == ref and it > 0 and rel <= 1e-4
        assert res / ref == pytest.approx(rel, rel=1e-6)
        assert np.abs(a - exact)[U].max() < 0.05
    # the trivial images: the start, 0 iterations, residual 0
    for trivial in (np.full(t.shape, 255, np.uint8), np.full(t.shape, 128, np.uint8)):
        a, it, rel = fm.pcg_warm(img, trivial, 1, 1e-5, 500, 1e-4, np.full(t.shape, 0.3))
        assert (it, rel) == (0, 0.0) and np.array_equal(a, tm.start_image(trivial, np.full(t.shape, 0.3)))


@functools.lru_cache(maxsize=None)
def _big(seed):
    full, at, work, mask = fm.full_scene(480, 640, 4, seed)
    return at, mask, fm.chain(full, work, mask), fm.chain(full, work, mask, warm=False)


@pytest.mark.parametrize("seed", [0, 1])
def test_warm_stops_sooner_than_cold_on_the_strand_scenes(seed):
    from gcn_grabcut.pipeline import nearest_upsample
    at, mask, warm, cold = _big(seed)
    assert warm["iters"] < cold["iters"]
    assert (warm["iters"], cold["iters"]) == (WARM_ITERS[seed], COLD_ITERS[seed])
    assert warm["rel"] <= 1e-4 and cold["rel"] <= 1e-4
    assert np.abs(warm["alpha"] - cold["alpha"]).max() < 0.02
    # the recorded quality ratio is the restatement's, and the full-size solve beats what it started from
    s_mask = fm.sad(nearest_upsample(mask, 480, 640), at)
    assert fm.sad(warm["alpha"], at) / s_mask == pytest.approx(RATIO[seed], abs=5e-4)
    assert fm.sad(warm["alpha"], at) < 0.5 * fm.sad(warm["alpha0_full"], at)


def test_recorded_tau_is_the_restatements():
    worst = 0.0
    for case in fm.WARM_CASES:
        full, t_full, a0 = fm.warm_case(*case)
        a, _, _ = fm.pcg_warm(full, t_full, 1, 1e-5, fm.FULL_MAX_ITER, 1e-4, a0)
        b, _, rel = fm.pcg_warm(full, t_full, 1, 1e-5, 20000, 1e-12, a0)
        assert rel <= 1e-12
        worst = max(worst, float(np.abs(a - b).max()))
    assert worst == pytest.approx(TAU_MEASURED, abs=5e-4)


# ---------------------------------------------------------------- the host side
def _no_device(monkeypatch):
    from gcn_grabcut import _engine

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_engine, "get_engine", boom)


def _noise(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng


def test_public_names():
    import gcn_grabcut
    import src.gcn_grabcut as shim
    from gcn_grabcut import pipeline as P
    for name in ("lift_trimap", "closed_form_matte_full", "trimap_matte_full", "trimap_matte_warm"):
        assert name in gcn_grabcut.__all__ and hasattr(gcn_grabcut, name) and hasattr(shim, name)
    assert P.CF_FULL_MAX_ITER == 2000 == fm.FULL_MAX_ITER
    d = {k: v.default for k, v in inspect.signature(gcn_grabcut.closed_form_matte_full).parameters.items()}
    assert list(d)[:3] == ["image", "mask", "full_image"]
    assert (d["radius"], d["eps"], d["band"], d["max_iter"], d["tol"]) == (P.CF_RADIUS, P.CF_EPS, P.CF_BAND, P.CF_MAX_ITER,
                                                                           P.CF_TOL) == fm.CF
    assert (d["grow"], d["full_max_iter"], d["return_info"]) == (0, 2000, False)
    d = {k: v.default for k, v in inspect.signature(gcn_grabcut.trimap_matte_full).parameters.items()}
    assert list(d)[:3] == ["image", "trimap", "full_image"] and (d["grow"], d["full_max_iter"]) == (0, 2000)
    # the warm solve is a function of its own: trimap_matte's parameter list is pinned (test_trimap_matte_cpu.py)
    cold, warm = (inspect.signature(f).parameters for f in (gcn_grabcut.trimap_matte, gcn_grabcut.trimap_matte_warm))
    assert "warm" not in cold and list(warm)[:3] == ["image", "trimap", "alpha0"]
    assert warm["alpha0"].default is inspect.Parameter.empty
    assert {k: v.default for k, v in warm.items() if k != "alpha0"} == {k: v.default for k, v in cold.items() if k != "alpha0"}
    assert list(inspect.signature(gcn_grabcut.lift_trimap).parameters)[:4] == ["trimap", "alpha", "full_shape", "grow"]
    m = gcn_grabcut.ClosedFormMatte()
    assert (m.full_resolution, m.grow, m.full_max_iter) == (False, 0, 2000)
    assert m.args() == (P.CF_RADIUS, P.CF_EPS, P.CF_BAND, P.CF_MAX_ITER, P.CF_TOL)


def test_warm_without_a_start_is_refused_before_any_device_call(monkeypatch):
    import torch
    from gcn_grabcut import trimap_matte_warm
    _no_device(monkeypatch)
    img, _ = _noise(12, 14, 0)
    t = np.full((12, 14), 128, np.uint8)
    with pytest.raises(ValueError, match="alpha0"):
        trimap_matte_warm(img, t, None)
    with pytest.raises(TypeError):
        trimap_matte_warm(img, t)
    for bad in (np.zeros((12, 13)), np.zeros((12, 14), np.uint8), np.full((12, 14), np.nan)):
        with pytest.raises(ValueError):
            trimap_matte_warm(img, t, bad)
    with pytest.raises(ValueError):
        trimap_matte_warm(img, t, np.zeros((12, 14)), tol=1.0)
    with pytest.raises(ValueError, match="alpha0"):
        _dead_engine().trimap_matte(torch.as_tensor(img[None]), torch.as_tensor(t[None]), 1, 1e-5, 10, 1e-4, warm=True)


@pytest.mark.parametrize("what", ["smaller", "too_large", "grow_neg", "grow_big", "grow_float", "alpha_shape", "alpha_int",
                                  "alpha_nan", "trimap_dtype", "trimap_ndim", "full_shape_len"])
def test_lift_trimap_refuses_bad_inputs_on_the_host(monkeypatch, what):
    from gcn_grabcut import lift_trimap
    _no_device(monkeypatch)
    t, a, full, grow = np.full((12, 14), 128, np.uint8), np.zeros((12, 14), np.float32), (24, 28), 0
    if what == "smaller":
        full = (24, 13)
    elif what == "too_large":
        full = (32769, 28)
    elif what == "grow_neg":
        grow = -1
    elif what == "grow_big":
        grow = 65
    elif what == "grow_float":
        grow = 1.5
    elif what == "alpha_shape":
        a = a[:, :13]
    elif what == "alpha_int":
        a = a.astype(np.uint8)
    elif what == "alpha_nan":
        a[2, 3] = np.nan
    elif what == "trimap_dtype":
        t = t.astype(np.int32)
    elif what == "trimap_ndim":
        t, a = t[None], a[None]
    elif what == "full_shape_len":
        full = (24, 28, 3)
    with pytest.raises(ValueError):
        lift_trimap(t, a, full, grow)


@pytest.mark.parametrize("what", ["full_smaller", "full_dtype", "grow", "full_iters", "radius", "tol", "small", "second_shape",
                                  "second_values"])
def test_full_chains_refuse_bad_inputs_on_the_host(monkeypatch, what):
    from gcn_grabcut import closed_form_matte_full, trimap_matte_full
    _no_device(monkeypatch)
    img, rng = _noise(12, 14, 0)
    full, _ = _noise(24, 28, 1)
    mask = (rng.random((12, 14)) > 0.5).astype(np.uint8)
    trimap = np.where(mask > 0, 255, 0).astype(np.uint8)
    kw = {}
    if what == "full_smaller":
        full = full[:11]
    elif what == "full_dtype":
        full = full.astype(np.float32)
    elif what == "grow":
        kw["grow"] = 65
    elif what == "full_iters":
        kw["full_max_iter"] = 0
    elif what == "radius":
        kw["radius"] = 9
    elif what == "tol":
        kw["tol"] = 1.0
    elif what == "small":
        img, mask, trimap = img[:2], mask[:2], trimap[:2]
    elif what == "second_shape":
        mask, trimap = mask[:, :13], trimap[:, :13]
    elif what == "second_values":
        mask, trimap = mask * 2, trimap.astype(np.float32)
    with pytest.raises(ValueError):
        closed_form_matte_full(img, mask, full, **kw)
    with pytest.raises(ValueError):
        trimap_matte_full(img, trimap, full, **kw)


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


@pytest.mark.parametrize("what", ["alpha_shape", "alpha_dtype", "trimap_dtype", "smaller", "grow", "nothing", "band"])
def test_engine_refuses_bad_tensors_before_any_call(what):
    import torch
    t, a = torch.full((2, 12, 14), 128, dtype=torch.uint8), torch.zeros(2, 12, 14)
    full, grow, kw = (24, 28), 0, {}
    if what == "alpha_shape":
        a = a[:1]
    elif what == "alpha_dtype":
        a = a.double()
    elif what == "trimap_dtype":
        t = t.int()
    elif what == "smaller":
        full = (11, 28)
    elif what == "grow":
        grow = 65
    elif what == "nothing":
        kw = dict(want_trimap=False, want_alpha0=False)
    if what == "band":
        with pytest.raises(ValueError):
            _dead_engine().closed_form_band(t, 65)
        with pytest.raises(ValueError):
            _dead_engine().closed_form_band(t.float(), 1)
        return
    with pytest.raises(ValueError):
        _dead_engine().lift_trimap(t, a, full, grow, **kw)


def test_closed_form_matte_full_resolution_arguments():
    from gcn_grabcut import ClosedFormMatte
    from gcn_grabcut.pipeline import _closed_form_args, _closed_form_full_args
    on = ClosedFormMatte(full_resolution=True)
    assert _closed_form_args(on, 50, 50, True) == (1, 1e-5, 1, 500, 1e-4)
    assert _closed_form_full_args(on) == (0, 2000) and _closed_form_full_args(ClosedFormMatte()) is None
    assert _closed_form_full_args(True) is None
    assert _closed_form_full_args(ClosedFormMatte(full_resolution=True, grow=3, full_max_iter=77)) == (3, 77)
    with pytest.raises(ValueError, match="full image"):
        _closed_form_args(on, 50, 50, False)
    with pytest.raises(ValueError, match="full_resolution=True"):      # the old refusal now names the opt-in
        _closed_form_args(ClosedFormMatte(), 50, 50, True)
    for bad in (dict(grow=-1), dict(grow=65), dict(grow=0.5), dict(full_max_iter=0), dict(full_max_iter=100001)):
        with pytest.raises(ValueError):
            _closed_form_full_args(ClosedFormMatte(full_resolution=True, **bad))


def test_pipeline_refuses_full_resolution_without_a_full_image_before_any_stage():
    from gcn_grabcut import ClosedFormMatte, GCNGrabCutPipeline
    pipe = GCNGrabCutPipeline.__new__(GCNGrabCutPipeline)

    class NoEngine:
        def __getattr__(self, name):
            raise AssertionError(f"stage {name} was reached")

    pipe._eng = NoEngine()
    img, _ = _noise(40, 50, 3)
    on = ClosedFormMatte(full_resolution=True)
    for call in (lambda: pipe.segment(img, matte=on), lambda: pipe.segment_bbox(img, (5, 5, 30, 20), matte=on),
                 lambda: pipe.segment_batch([img, img], matte=on),
                 lambda: pipe.segment(img, matte=on, full_image=img, foreground=True),
                 lambda: pipe.segment(img, matte=ClosedFormMatte(full_resolution=True, grow=99), full_image=img)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("name,n", [("ggc_trimap_matte_warm", 17), ("ggc_lift_trimap", 12), ("ggc_closed_form_band", 8)])
def test_ctypes_rows_match_the_header(name, n):
    import ctypes
    from gcn_grabcut import _native
    header = (ROOT / "include" / "ggc.h").read_text()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", body, flags=re.S)
    assert m, f"{name} is not declared in include/ggc.h"
    params = [p.strip() for p in m.group(1).split(",")]
    row = _native.SIGNATURES[name]
    assert len(params) == len(row) == n
    for p, c in zip(params, row):
        want = ctypes.c_void_p if "*" in p or "ggc_stream" in p else (ctypes.c_float if p.startswith("float") else ctypes.c_int)
        assert c is want, (p, c)
    assert hasattr(_native.load_library(), name)
    assert int(re.search(r"#define GGC_VERSION (\d+)", header).group(1)) >= 402
    if name == "ggc_trimap_matte_warm":       # the arguments of ggc_trimap_matte
        assert row == _native.SIGNATURES["ggc_trimap_matte"]


def test_header_states_the_scratch_of_the_new_entries():
    header = (ROOT / "include" / "ggc.h").read_text()
    for name in ("ggc_trimap_matte_warm", "ggc_lift_trimap", "ggc_closed_form_band"):
        comment = header[:header.index(f"int {name}(")].rsplit("/*", 1)[1]
        assert "Scratch:" in comment, name


# ---------------------------------------------------------------- command lines
def _run(script, *argv):
    return subprocess.run([sys.executable, str(ROOT / script), *argv], capture_output=True, text=True, timeout=120)


def test_inference_cli_offers_the_full_size_solve(tmp_path):
    r = _run("inference.py", "--help")
    assert r.returncode == 0
    for word in ("closed-form-full", "--cf-grow", "--cf-full-iters"):
        assert word in r.stdout
    r = _run("inference.py", "--image", str(tmp_path / "x.png"), "--matte-method", "closed-form-full", "--save", "alpha")
    assert r.returncode == 2 and "--full-res" in r.stderr
    r = _run("inference.py", "--image", str(tmp_path / "x.png"), "--matte-method", "closed-form-full", "--full-res",
             "--cf-grow", "65", "--save", "alpha")
    assert r.returncode == 2 and "grow" in r.stderr
    r = _run("inference.py", "--image", str(tmp_path / "x.png"), "--full-res", "--matte-method", "closed-form", "--save",
             "alpha")
    assert r.returncode == 2 and "full-res" in r.stderr and "closed-form-full" in r.stderr


def test_matte_cli_offers_a_full_image(tmp_path):
    r = _run("matte.py", "--help")
    assert r.returncode == 0
    for word in ("--full-image", "--full-images", "--cf-grow", "--cf-full-iters"):
        assert word in r.stdout
    r = _run("matte.py", "--image", "a.png", "--trimap", "t.png", "--full-images", str(tmp_path))
    assert r.returncode == 2 and "--full-image" in r.stderr
    r = _run("matte.py", "--input", str(tmp_path), "--trimaps", str(tmp_path), "--full-image", "a.png")
    assert r.returncode == 2 and "--full-images" in r.stderr
    r = _run("matte.py", "--image", "a.png", "--trimap", "t.png", "--full-image", "b.png", "--cf-grow", "65")
    assert r.returncode == 2 and "grow" in r.stderr
