"""The full-resolution banded cut without a GPU: the numpy restatement of ggc_lift_labels (tests/full_cut_ref.py) against
a per-pixel loop, the default band, every host-side refusal of the new public functions and options, and the quality
claim of DESIGN.md §5.18 on the CPU oracle, whose totals the GPU test (test_full_cut_gpu.py) holds the device to."""
import functools
import inspect
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import full_cut_ref as fc

ROOT = Path(__file__).resolve().parent.parent

# Wrong pixels against the truth summed over the six 240x320 scenes (good working mask, shifted working mask), measured
# on the restatement and the CPU oracle (tools/full_cut_study.py --table).  The GPU test imports them.
LIFTED_TOTALS = (2276, 7110)
GUIDED_TOTALS = (525, 1157)
CUT_TOTALS = (5, 5)            # default band 6, n_iter 1, seed 0
# 96x128 from 24x32, seed 30000, good mask: a small ellipse thinner than twice the band is lost (--thin)
THIN_BAND6, THIN_BAND2 = 149, 3


@functools.lru_cache(maxsize=None)
def _totals():
    return fc.study_totals((None,))


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape,full", [((5, 7), (5, 7)), ((5, 7), (13, 18)), ((6, 4), (22, 9))])
@pytest.mark.parametrize("band", [0, 1, 3])
def test_restatement_equals_brute_force(shape, full, band):
    rng = np.random.default_rng(shape[0] * 100 + full[1] + band)
    for mask in ((rng.random(shape) < 0.5).astype(np.uint8), np.zeros(shape, np.uint8), np.ones(shape, np.uint8)):
        got, want = fc.lift_labels(mask, full, band), fc.brute_force_lift_labels(mask, full, band)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert got[0].dtype == np.uint8 and got[0].max() <= 3 and np.array_equal(got[0] & 1, got[1])
    labels, m1 = fc.lift_labels(np.ones(shape, np.uint8), full, band)
    assert (labels == 1).all() and (m1 == 1).all()          # no edge, no band: the degenerate case GrabCut hands back


def test_identity_size_keeps_the_mask():
    mask = (np.random.default_rng(3).random((9, 11)) < 0.4).astype(np.uint8) * 255
    labels, m1 = fc.lift_labels(mask, (9, 11), 0)
    assert np.array_equal(m1, mask != 0)
    assert np.array_equal(labels >> 1, fc.unknown_band(mask, 0))


def test_default_band():
    from gcn_grabcut._engine import default_full_cut_band
    for shape, full, want in (((60, 80), (240, 320), 6), ((24, 32), (96, 128), 6), ((10, 10), (10, 10), 2),
                              ((10, 10), (15, 10), 3), ((100, 100), (100, 199), 3), ((300, 400), (1200, 1600), 6),
                              ((10, 10), (1000, 1000), 64), ((72, 96), (216, 288), 5)):
        assert default_full_cut_band(shape, full) == fc.default_band(shape, full) == want


# ---------------------------------------------------------------- host-side refusals
def _no_device(monkeypatch):
    from gcn_grabcut import _engine

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_engine, "get_engine", boom)


def test_public_names():
    import gcn_grabcut
    import src.gcn_grabcut as shim
    from gcn_grabcut import pipeline as P
    for name in ("lift_labels", "cut_mask_full", "FullCut"):
        assert name in gcn_grabcut.__all__ and hasattr(gcn_grabcut, name) and hasattr(shim, name)
    d = {k: v.default for k, v in inspect.signature(gcn_grabcut.cut_mask_full).parameters.items()}
    assert list(d) == ["mask", "full_image", "band", "n_iter", "seed", "color_space", "min_area_ratio", "keep_largest",
                       "return_labels", "device"]
    assert (d["band"], d["n_iter"], d["seed"], d["color_space"], d["min_area_ratio"], d["keep_largest"],
            d["return_labels"]) == (None, 1, 0, "rgb", 0.002, False, False)
    assert list(inspect.signature(gcn_grabcut.lift_labels).parameters) == ["mask", "full_shape", "band", "device"]
    f = gcn_grabcut.FullCut()
    assert (f.band, f.n_iter) == (None, 1)
    assert isinstance(P.FULL_CUT_PIXELS, int) and P.FULL_CUT_PIXELS >= 1
    for fn in ("segment", "segment_bbox", "segment_batch_device"):
        assert inspect.signature(getattr(gcn_grabcut.GCNGrabCutPipeline, fn)).parameters["full_cut"].default is False


@pytest.mark.parametrize("what", ["smaller", "too_large", "band_neg", "band_big", "band_float", "band_bool",
                                  "iters_zero", "iters_big", "colour", "mask_values", "mask_ndim", "mask_float", "full_dtype"])
def test_cut_mask_full_refuses_bad_inputs_on_the_host(monkeypatch, what):
    from gcn_grabcut import cut_mask_full
    _no_device(monkeypatch)
    mask = np.zeros((12, 14), np.uint8)
    mask[3:9, 4:10] = 1
    full = np.zeros((24, 28, 3), np.uint8)
    kw = {}
    if what == "smaller":
        full = full[:, :13]
    elif what == "too_large":
        full = np.zeros((12, 32769, 3), np.uint8)
    elif what == "band_neg":
        kw["band"] = -1
    elif what == "band_big":
        kw["band"] = 65
    elif what == "band_float":
        kw["band"] = 1.5
    elif what == "band_bool":
        kw["band"] = True
    elif what == "iters_zero":
        kw["n_iter"] = 0
    elif what == "iters_big":
        kw["n_iter"] = 101
    elif what == "colour":
        kw["color_space"] = "xyz"
    elif what == "mask_values":
        mask = mask * 2
    elif what == "mask_ndim":
        mask = mask[None]
    elif what == "mask_float":
        mask = mask.astype(np.float32)
    elif what == "full_dtype":
        full = full.astype(np.float32)
    with pytest.raises(ValueError):
        cut_mask_full(mask, full, **kw)


@pytest.mark.parametrize("what", ["smaller", "too_large", "band_neg", "band_big", "band_float", "mask_values", "full_shape_len"])
def test_lift_labels_refuses_bad_inputs_on_the_host(monkeypatch, what):
    from gcn_grabcut import lift_labels
    _no_device(monkeypatch)
    mask, full, band = np.ones((12, 14), np.uint8), (24, 28), 2
    if what == "smaller":
        full = (11, 28)
    elif what == "too_large":
        full = (24, 32769)
    elif what == "band_neg":
        band = -1
    elif what == "band_big":
        band = 65
    elif what == "band_float":
        band = 0.5
    elif what == "mask_values":
        mask = mask * 255
    elif what == "full_shape_len":
        full = (24, 28, 3)
    with pytest.raises(ValueError):
        lift_labels(mask, full, band)


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


@pytest.mark.parametrize("what", ["dtype", "ndim", "smaller", "band", "nothing"])
def test_engine_refuses_bad_tensors_before_any_call(what):
    import torch
    m, full, band, kw = torch.ones(2, 12, 14, dtype=torch.uint8), (24, 28), 3, {}
    if what == "dtype":
        m = m.float()
    elif what == "ndim":
        m = m[0]
    elif what == "smaller":
        full = (24, 13)
    elif what == "band":
        band = 65
    elif what == "nothing":
        kw = dict(want_labels=False, want_mask=False)
    with pytest.raises(ValueError):
        _dead_engine().lift_labels(m, full, band, **kw)


def test_check_full_cut_args_accepts_the_limits():
    from gcn_grabcut._engine import check_full_cut_args
    check_full_cut_args((1, 12, 14), (12, 14), 0)
    check_full_cut_args((3, 12, 14), (32768, 8191), 64, 100, "LAB")
    check_full_cut_args((0, 1, 1), (1, 1), 1, 1, "hsv")
    with pytest.raises(ValueError, match="2\\^28"):           # ggc_grabcut's limit, refused before the lift runs
        check_full_cut_args((1, 12, 14), (16384, 16384), 1)


def test_full_cut_option_arguments():
    from gcn_grabcut import ClosedFormMatte, FullCut
    from gcn_grabcut.pipeline import _full_cut_args
    assert _full_cut_args(False, True, None) is None and _full_cut_args(None, False, None) is None
    assert _full_cut_args(True, True, None) == (None, 1)
    assert _full_cut_args(FullCut(band=2, n_iter=2), True, True, (60, 80), (240, 320)) == (2, 2)
    assert _full_cut_args(True, True, ClosedFormMatte()) == (None, 1)           # that pairing is refused elsewhere, as before
    with pytest.raises(ValueError, match="full image"):
        _full_cut_args(True, False, None)
    with pytest.raises(ValueError, match=r"closed_form_matte\(full_image, result\.full\.binary_mask\)"):
        _full_cut_args(True, True, ClosedFormMatte(full_resolution=True))
    for bad in (FullCut(band=-1), FullCut(band=65), FullCut(band=1.5), FullCut(n_iter=0), FullCut(n_iter=101), "cut", 1):
        with pytest.raises(ValueError):
            _full_cut_args(bad, True, None)


def test_pipeline_refuses_full_cut_before_any_stage():
    from gcn_grabcut import ClosedFormMatte, FullCut, GCNGrabCutPipeline
    pipe = GCNGrabCutPipeline.__new__(GCNGrabCutPipeline)

    class NoEngine:
        def __getattr__(self, name):
            raise AssertionError(f"stage {name} was reached")

    pipe._eng = NoEngine()
    img = np.random.default_rng(3).integers(0, 256, (40, 50, 3), dtype=np.uint8)
    on = ClosedFormMatte(full_resolution=True)
    for call in (lambda: pipe.segment(img, full_cut=True), lambda: pipe.segment_bbox(img, (5, 5, 30, 20), full_cut=True),
                 lambda: pipe.segment_batch([img, img], full_cut=True),
                 lambda: pipe.segment(img, full_image=img, full_cut=True, matte=on),
                 lambda: pipe.segment_bbox(img, (5, 5, 30, 20), full_image=img, full_cut=True, matte=on),
                 lambda: pipe.segment_batch([img, img], full_images=[img, img], full_cut=True, matte=on),
                 lambda: pipe.segment(img, full_image=img, full_cut=FullCut(band=99))):
        with pytest.raises(ValueError):
            call()


def test_ctypes_row_and_header():
    import ctypes
    from gcn_grabcut import _native
    header = (ROOT / "include" / "ggc.h").read_text()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bggc_lift_labels\s*\(([^;]*?)\)\s*;", body, flags=re.S)
    assert m, "ggc_lift_labels is not declared in include/ggc.h"
    params = [p.strip() for p in m.group(1).split(",")]
    row = _native.SIGNATURES["ggc_lift_labels"]
    assert len(params) == len(row) == 11
    for p, c in zip(params, row):
        assert c is (ctypes.c_void_p if "*" in p or "ggc_stream" in p else ctypes.c_int), (p, c)
    assert hasattr(_native.load_library(), "ggc_lift_labels")
    assert int(re.search(r"#define GGC_VERSION (\d+)", header).group(1)) >= 403
    comment = header[:header.index("int ggc_lift_labels(")].rsplit("/*", 1)[1]
    assert "Scratch:" in comment and "Does not synchronise" in comment


# ---------------------------------------------------------------- quality, on the CPU oracle
def test_banded_cut_beats_the_guided_upsample_tenfold(oracle):
    rows = _totals()
    cut, guided, lifted = rows[("cut", None)], rows["guided"], rows["lifted"]
    print(f"lifted {lifted}  guided {guided}  cut {cut}")
    for j in (0, 1):                                       # good working mask, shifted working mask
        assert 10 * cut[j] <= guided[j]
        assert cut[j] < lifted[j]


def test_recorded_totals(oracle):
    rows = _totals()
    assert rows["lifted"] == LIFTED_TOTALS and rows["guided"] == GUIDED_TOTALS and rows[("cut", None)] == CUT_TOTALS


def test_thin_component_is_lost_at_a_wide_band(oracle):
    """Documented behaviour, not a defect of the code: a component of the lifted mask thinner than twice the band keeps
    no definite pixel, and the cut may delete it."""
    full, truth, _ = fc.scene(96, 128, 30000, 4)
    good, _ = fc.working_masks(truth, 4)
    assert fc.default_band(good.shape, (96, 128)) == 6
    wide, narrow = fc.wrong(fc.chain(good, full, 6), truth), fc.wrong(fc.chain(good, full, 2), truth)
    print(f"band 6: {wide}  band 2: {narrow}")
    assert wide >= 100 and narrow <= 10
    assert (wide, narrow) == (THIN_BAND6, THIN_BAND2)


def test_trivial_masks_come_back_as_lifted(oracle):
    full, _, _ = fc.scene(48, 64, 30001, 4)
    for mask in (np.zeros((12, 16), np.uint8), np.ones((12, 16), np.uint8)):
        assert np.array_equal(fc.chain(mask, full), np.broadcast_to(mask[:1, :1], (48, 64)))


# ---------------------------------------------------------------- command line
def _run(script, *argv):
    return subprocess.run([sys.executable, str(ROOT / script), *argv], capture_output=True, text=True, timeout=120)


def test_inference_cli_offers_the_full_cut(tmp_path):
    r = _run("inference.py", "--help")
    assert r.returncode == 0
    for word in ("--full-mask", "--full-cut-band", "--full-cut-iters"):
        assert word in r.stdout
    r = _run("inference.py", "--image", str(tmp_path / "x.png"), "--full-mask", "cut", "--save", "mask")
    assert r.returncode == 2 and "--full-res" in r.stderr
    r = _run("inference.py", "--image", str(tmp_path / "x.png"), "--full-res", "--full-mask", "cut", "--matte-method",
             "closed-form-full", "--save", "alpha")
    assert r.returncode == 2 and "closed-form-full" in r.stderr
    r = _run("inference.py", "--image", str(tmp_path / "x.png"), "--full-res", "--full-mask", "cut", "--full-cut-band", "65")
    assert r.returncode == 2 and "band" in r.stderr
