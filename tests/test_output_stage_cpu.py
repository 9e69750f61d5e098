"""The post-GrabCut output stage of the pipeline (pipeline._OutputPlan, pipeline._OutputStage) without a GPU: the engine
calls it issues, their scalar arguments, the slices it hands them and the keys of the result, for every option set,
against call lists written out here from the stage's specification (clean-up, composition, matte, foreground colours,
then the full-resolution outputs by the full cut, the full-size closed form or the guided upsample)."""
from types import SimpleNamespace

import pytest
import torch

from gcn_grabcut import ClosedFormMatte, FullCut, GrabCutConfig
from gcn_grabcut import pipeline
from gcn_grabcut.pipeline import _OutputPlan, _OutputStage

B, H, W, H1, W1 = 3, 8, 10, 16, 20
SEED, MIN_AREA, KEEP, RADIUS, EPS = 7, 0.01, True, 3, 1e-3
PIPE = SimpleNamespace(gc_config=GrabCutConfig(color_space="LAB", seed=SEED))
CF = (1, 1e-5, 1, 500, 1e-4)                      # ClosedFormMatte()'s radius, eps, band, max_iter, tol
FG = (5e-3, 1.0, 2000, 1e-6)                      # ForegroundColours()'s eps_r, omega, max_iter, tol


def _t(x):
    """A tensor as (index of its first image in the batch buffer it is a slice of, shape); None stays None."""
    if x is None:
        return None
    per_image = 1
    for v in x.shape[1:]:
        per_image *= int(v)
    assert x.storage_offset() % per_image == 0
    return (x.storage_offset() // per_image, tuple(x.shape))


class Recorder:
    """Stands in for the engine: every entry the stage may call records (name, scalar arguments, input tensors, out=
    tensors) and computes nothing."""

    def __init__(self):
        self.calls = []

    def empty(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype)

    def _rec(self, name, scalars, tensors, out):
        self.calls.append((name, tuple(scalars), tuple(_t(t) for t in tensors), tuple(_t(o) for o in out)))

    def clean_mask(self, mask, min_area_ratio=0.002, keep_largest=False, out=None):
        self._rec("clean_mask", (min_area_ratio, keep_largest), (mask,), (out,))

    def compose(self, bgr, binary, alpha=0.45, tint_bgr=(100, 220, 0), out=None):
        self._rec("compose", (alpha, tint_bgr), (bgr, binary), out)

    def alpha_matte(self, bgr, binary, radius=4, eps=1e-4, want_rgba=False, out=None):
        self._rec("alpha_matte", (radius, eps, want_rgba), (bgr, binary), out)

    def closed_form_matte(self, bgr, binary, radius, eps, band, max_iter, tol, want_rgba=False, out=None):
        self._rec("closed_form_matte", (radius, eps, band, max_iter, tol, want_rgba), (bgr, binary), out)

    def estimate_foreground(self, bgr, alpha, eps_r, omega, max_iter, tol, want_rgba=False, out=None):
        self._rec("estimate_foreground", (eps_r, omega, max_iter, tol, want_rgba), (bgr, alpha), out)

    def upsample_matte(self, bgr, binary, bgr_full, radius=4, eps=1e-4, want_alpha=True, want_binary=True, want_rgba=False,
                       out=None):
        self._rec("upsample_matte", (radius, eps), (bgr, binary, bgr_full), out)

    def cut_mask_full(self, binary, bgr_full, band, n_iter=1, seed=0, color_space="rgb", min_area_ratio=0.002,
                      keep_largest=False, out=None, max_pixels=None, want_labels=False):
        self._rec("cut_mask_full", (band, n_iter, seed, color_space, min_area_ratio, keep_largest, max_pixels, want_labels),
                  (binary, bgr_full), (out,))

    def closed_form_band(self, binary, band):
        self._rec("closed_form_band", (band,), (binary,), ())
        return torch.zeros(tuple(binary.shape), dtype=torch.uint8)

    def closed_form_full(self, bgr, trimap, alpha, bgr_full, radius, eps, grow, max_iter, tol, out=None):
        self._rec("closed_form_full", (radius, eps, grow, max_iter, tol), (bgr, trimap, alpha, bgr_full), out)


# ---------------------------------------------------------------- the calls, for images lo:lo+n
def _small(lo, n, *c):
    return (lo, (n, H, W, *c))


def _big(lo, n, *c):
    return (lo, (n, H1, W1, *c))


def clean(lo, n):
    return ("clean_mask", (MIN_AREA, KEEP), (_small(lo, n),), (_small(lo, n),))


def compose(lo, n):
    return ("compose", (0.45, (100, 220, 0)), (_small(lo, n, 3), _small(lo, n)), (_small(lo, n, 3), _small(lo, n, 4)))


def compose_full(lo, n):
    return ("compose", (0.45, (100, 220, 0)), (_big(lo, n, 3), _big(lo, n)), (_big(lo, n, 3), _big(lo, n, 4)))


def guided(lo, n):
    return ("alpha_matte", (RADIUS, EPS, True), (_small(lo, n, 3), _small(lo, n)), (_small(lo, n), _small(lo, n, 4)))


def closed_form(lo, n):
    return ("closed_form_matte", (*CF, False), (_small(lo, n, 3), _small(lo, n)), (_small(lo, n), _small(lo, n, 4)))


def foreground(lo, n):
    return ("estimate_foreground", (*FG, False), (_small(lo, n, 3), _small(lo, n)), (_small(lo, n, 3), _small(lo, n, 4)))


def upsample(lo, n, alpha, mask):
    """ggc_upsample_matte's outputs: alpha and rgba_soft together or not at all, the mask unless the full cut makes it."""
    return ("upsample_matte", (RADIUS, EPS), (_small(lo, n, 3), _small(lo, n), _big(lo, n, 3)),
            (_big(lo, n) if alpha else None, _big(lo, n) if mask else None, _big(lo, n, 4) if alpha else None))


def full_cut(lo, n, band, n_iter):
    return ("cut_mask_full", (band, n_iter, SEED + lo, "lab", MIN_AREA, KEEP, pipeline.FULL_CUT_PIXELS, False),
            (_small(lo, n), _big(lo, n, 3)), (_big(lo, n),))


def band_trimap(lo, n):
    return ("closed_form_band", (CF[2],), (_small(lo, n),), ())


def full_solve(lo, n, grow, full_max_iter):
    # the band's trimap is a tensor of its own, so it starts at 0 whatever lo is
    return ("closed_form_full", (CF[0], CF[1], grow, full_max_iter, CF[4]),
            (_small(lo, n, 3), _small(0, n), _small(lo, n), _big(lo, n, 3)), (_big(lo, n), _big(lo, n, 4)))


# name: (options, with a full image, the calls after clean-up and working-size composition, the optional keys of the result,
#        the keys of result["full"])
CASES = {
    "nothing": (dict(compose=False), False, lambda lo, n: [], set(), None),
    "compose": (dict(), False, lambda lo, n: [], {"overlay", "rgba"}, None),
    "matte": (dict(matte=True), False, lambda lo, n: [guided(lo, n)], {"overlay", "rgba", "alpha", "rgba_soft"}, None),
    "closed_form": (dict(matte=ClosedFormMatte()), False, lambda lo, n: [closed_form(lo, n)],
                    {"overlay", "rgba", "alpha", "rgba_soft"}, None),
    "matte_foreground": (dict(matte=True, foreground=True), False, lambda lo, n: [guided(lo, n), foreground(lo, n)],
                         {"overlay", "rgba", "alpha", "rgba_soft", "foreground", "rgba_clean"}, None),
    "full": (dict(), True, lambda lo, n: [upsample(lo, n, False, True), compose_full(lo, n)],
             {"overlay", "rgba", "full"}, {"binary_mask", "overlay", "rgba"}),
    "full_matte": (dict(matte=True), True, lambda lo, n: [guided(lo, n), upsample(lo, n, True, True), compose_full(lo, n)],
                   {"overlay", "rgba", "alpha", "rgba_soft", "full"}, {"binary_mask", "overlay", "rgba", "alpha", "rgba_soft"}),
    # the default band at twice the working size: ceil(1.5 * 2) = 3
    "full_cut": (dict(full_cut=True), True, lambda lo, n: [full_cut(lo, n, 3, 1), compose_full(lo, n)],
                 {"overlay", "rgba", "full"}, {"binary_mask", "overlay", "rgba"}),
    "full_matte_cut": (dict(matte=True, full_cut=FullCut(band=2, n_iter=2)), True,
                       lambda lo, n: [guided(lo, n), upsample(lo, n, True, False), full_cut(lo, n, 2, 2), compose_full(lo, n)],
                       {"overlay", "rgba", "alpha", "rgba_soft", "full"}, {"binary_mask", "overlay", "rgba", "alpha", "rgba_soft"}),
    "full_closed_form": (dict(matte=ClosedFormMatte(full_resolution=True, grow=1, full_max_iter=7)), True,
                         lambda lo, n: [closed_form(lo, n), band_trimap(lo, n), full_solve(lo, n, 1, 7), compose_full(lo, n)],
                         {"overlay", "rgba", "alpha", "rgba_soft", "full"},
                         {"binary_mask", "overlay", "rgba", "alpha", "rgba_soft"}),
}
FRONT_KEYS = {"binary_mask", "trimap", "segments", "graphs", "probs", "gc_mask"}


def _stage(name, final_mask=None):
    options, with_full, _, _, _ = CASES[name]
    eng = Recorder()
    bgr = torch.zeros(B, H, W, 3, dtype=torch.uint8)
    full_bgr = torch.zeros(B, H1, W1, 3, dtype=torch.uint8) if with_full else None
    plan = _OutputPlan.of(PIPE, bgr.shape, None if full_bgr is None else full_bgr.shape, min_area_ratio=MIN_AREA,
                          keep_largest=KEEP, matte_radius=RADIUS, matte_eps=EPS, **options)
    return eng, _OutputStage(eng, plan, bgr, full_bgr, final_mask=final_mask)


def _head(name, lo, n):
    return [clean(lo, n)] + ([compose(lo, n)] if CASES[name][0].get("compose", True) else [])


@pytest.mark.parametrize("name", list(CASES))
def test_run_issues_the_specified_calls_whole_and_split(name):
    tail = CASES[name][2]
    binary = torch.zeros(B, H, W, dtype=torch.uint8)
    eng, stage = _stage(name)
    stage.run(eng, 0, 3, binary)
    assert eng.calls == _head(name, 0, 3) + tail(0, 3)
    eng, stage = _stage(name)
    stage.run(eng, 0, 1, binary[0:1])
    stage.run(eng, 1, 3, binary[1:3])
    assert eng.calls == _head(name, 0, 1) + tail(0, 1) + _head(name, 1, 2) + tail(1, 2)
    for call in eng.calls:                                    # image b of the full cut runs on seed + b
        if call[0] == "cut_mask_full":
            assert call[1][2] == SEED + call[2][0][0]


@pytest.mark.parametrize("name", list(CASES))
def test_from_mask_skips_the_clean_up_and_the_working_size_composition(name):
    """segment_bbox's entry: GrabCut's mask is final and the overlay is GrabCut's own."""
    options, with_full, tail, _, full_keys = CASES[name]
    final = torch.zeros(B, H, W, dtype=torch.uint8)
    eng, stage = _stage(name, final_mask=final)
    stage.from_mask(eng, 0, 1)
    stage.from_mask(eng, 1, 3)
    assert eng.calls == tail(0, 1) + tail(1, 2)
    assert stage.cleaned is final and "overlay" not in stage.out and "rgba" not in stage.out
    assert (set(stage.out["full"]) == full_keys) if with_full else ("full" not in stage.out)


@pytest.mark.parametrize("name", list(CASES))
def test_result_has_the_keys_of_the_options(name):
    _, _, _, optional, full_keys = CASES[name]
    eng, stage = _stage(name)
    front = dict(trimap=1, segments=2, graphs=3, probs=4, gc_mask=5)
    out = stage.result(**front)
    assert set(out) == FRONT_KEYS | optional
    assert out["binary_mask"] is stage.cleaned and all(out[k] == v for k, v in front.items())
    assert tuple(out["binary_mask"].shape) == (B, H, W) and out["binary_mask"].dtype == torch.uint8
    if full_keys is not None:
        assert set(out["full"]) == full_keys
        assert all(tuple(v.shape[:3]) == (B, H1, W1) for v in out["full"].values())
        assert out["full"]["binary_mask"].dtype == torch.uint8
    for k in ("alpha", "rgba_soft", "foreground", "rgba_clean", "overlay", "rgba"):
        if k in out:
            assert tuple(out[k].shape[:3]) == (B, H, W) and out[k].dtype == (torch.float32 if k == "alpha" else torch.uint8)
    state = dict(gc_binary=6, bgd=7, fgd=8, gc_image=9)
    assert set(stage.result(**front, state=state)) == FRONT_KEYS | optional | set(state)


def test_full_cut_pixels_is_read_when_the_stage_runs(monkeypatch):
    eng, stage = _stage("full_cut")
    monkeypatch.setattr(pipeline, "FULL_CUT_PIXELS", 12345)
    stage.run(eng, 0, 3, torch.zeros(B, H, W, dtype=torch.uint8))
    cut = [c for c in eng.calls if c[0] == "cut_mask_full"]
    assert len(cut) == 1 and cut[0][1][6] == 12345


def test_plan_refuses_in_one_order_and_before_it_touches_the_pipeline():
    """A call that is wrong in several ways: hints, closed-form matte, guided matte, full image, foreground, full-size
    closed form, full cut.  The pipeline object (here one without a GrabCutConfig) is read only after all of them."""
    shape, full = (2, 40, 50, 3), (2, 80, 100, 3)
    bad_cf, bad_full_cf = ClosedFormMatte(eps=0.0), ClosedFormMatte(full_resolution=True, grow=99)
    for message, full_shape, options in (
            ("hint_region", None, dict(geodesic=True, hint_region=True, matte=bad_cf)),
            ("eps", None, dict(matte=bad_cf, foreground="yes")),
            ("radius", (2, 30, 100, 3), dict(matte=True, matte_radius=65)),
            ("full_bgr", (2, 30, 100, 3), dict(matte=True, foreground=True)),
            ("foreground", full, dict(matte=True, foreground=True, full_cut=FullCut(band=99))),
            ("grow", full, dict(matte=bad_full_cf, full_cut=True)),
            ("full_cut", None, dict(full_cut=True)),
            ("band", full, dict(full_cut=FullCut(band=99)))):
        with pytest.raises(ValueError, match=message):
            _OutputPlan.of(object(), shape, full_shape, **options)
    with pytest.raises(ValueError, match="foreground"):          # the full images are given but not read yet
        _OutputPlan.of(object(), shape, True, matte=True, foreground=True, full_cut=FullCut(band=99))
    with pytest.raises(AttributeError):                           # nothing to refuse: now the pipeline is read
        _OutputPlan.of(object(), shape, full, matte=True, full_cut=True)
    with pytest.raises(ValueError, match="color_space"):
        _OutputPlan.of(SimpleNamespace(gc_config=GrabCutConfig(color_space="xyz")), shape, None)
    plan = _OutputPlan.of(PIPE, shape, full, matte=True, full_cut=True)
    assert (plan.mat, plan.cfm, plan.cff, plan.fmat, plan.fga, plan.fcut) == ((4, 1e-4), None, None, (4, 1e-4), None, (None, 1))
    assert (plan.seed, plan.color_space, plan.compose, plan.min_area_ratio, plan.keep_largest) == (SEED, "lab", True, 0.002, False)
