"""The four matte errors (SAD, MSE, gradient, connectivity), without a GPU: the restatement in matte_eval_ref.py against
an independent brute force (BFS components, 81-tap loops), the hand case and the identities the definition gives, and
the host-side checks, scaling arithmetic and command-line refusals that need no device."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from matte_eval_ref import (blocky_levels, brute_force_errors, conventional, fading_levels, matte_errors_ref, random_levels,
                            threshold_set, tie_case, to_levels)

ROOT = Path(__file__).resolve().parent.parent
INTS = ("n", "sad", "sse", "conn")


def _brute_cases():
    """24 pairs up to 24 x 31: random levels with pixels at every k, blocky images with equal-area ties, mixtures."""
    rng = np.random.default_rng(2009)
    shapes = [(1, 1), (1, 13), (11, 1), (2, 2), (5, 9), (7, 12), (9, 9), (13, 8), (16, 16), (17, 23), (24, 31), (24, 31)]
    out = []
    for i, (h, w) in enumerate(shapes):
        out.append((f"random{h}x{w}", random_levels(rng, h, w), random_levels(rng, h, w), None))
    for i, (h, w) in enumerate([(7, 11), (11, 15), (12, 12), (15, 19), (19, 23), (24, 31), (23, 31), (24, 30)]):
        g = blocky_levels(rng, h, w)
        a = g.copy() if i % 2 == 0 else blocky_levels(rng, h, w)
        drop = rng.random((h, w)) < 0.08                             # a few pixels lowered: components split unevenly
        a[drop] = (a[drop] // 2).astype(np.uint8)
        out.append((f"blocky{h}x{w}", a, g, None))
    for h, w in [(10, 14), (24, 31)]:
        a, g = random_levels(rng, h, w), blocky_levels(rng, h, w, 4)
        out.append((f"mixed{h}x{w}", a, g, (rng.random((h, w)) < 0.5).astype(np.uint8)))
    a, g = tie_case()
    out.append(("tie", a, g, None))
    out.append(("fading", fading_levels(9, 20, 120), fading_levels(9, 20, 200), None))
    return out


BRUTE = _brute_cases()


def test_there_are_enough_brute_force_cases_and_they_cover_every_level_and_ties():
    assert len(BRUTE) >= 20
    name, a, g, _ = next(c for c in BRUTE if c[0] == "random24x31")
    assert all(threshold_set(a, g, k).any() for k in range(1, 11))
    from scipy import ndimage
    ties = 0
    for name, a, g, _ in BRUTE:
        if not name.startswith("blocky"):
            continue
        for k in range(1, 11):
            lab, n = ndimage.label(threshold_set(a, g, k))
            area = np.bincount(lab.ravel())[1:]
            ties += int(n > 1 and (area == area.max()).sum() > 1)
    assert ties >= 5, ties


@pytest.mark.parametrize("name,a,g,region", BRUTE, ids=[c[0] for c in BRUTE])
def test_restatement_matches_an_independent_brute_force(name, a, g, region):
    got, want = matte_errors_ref(a, g, region), brute_force_errors(a, g, region)
    assert np.array_equal(got["levels"], want["levels"])
    for k in INTS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert abs(got["grad"] - want["grad"]) <= 1e-12 * (1.0 + want["grad"]), (got["grad"], want["grad"])


def test_hand_case():
    a, g = tie_case()
    e = matte_errors_ref(a, g)
    assert (e["n"], e["sad"], e["sse"], e["conn"]) == (45, 408, 41616, 4080)
    lev = e["levels"]
    assert (lev[1:3, 1:3] == 10).all() and (lev[1:3, 5:7] == 0).all()        # the first square wins the tie
    assert lev.sum() == 40


def test_first_failure_not_the_last_level_that_holds():
    """The Omega_k need not be nested: a pixel outside Omega_1 has lev 0 even when it lies in a later Omega_k."""
    g = np.zeros((3, 12), np.uint8)
    g[1, 0:5] = 60                                                   # five pixels at levels 1..2
    g[1, 7:10] = 255                                                 # three pixels at every level
    e = matte_errors_ref(g, g)
    assert (e["levels"][1, 7:10] == 0).all() and (e["levels"][1, 0:5] == 2).all()


def _identity_pairs():
    rng = np.random.default_rng(5)
    a, g = tie_case()
    return [(a, g), (random_levels(rng, 14, 19), random_levels(rng, 14, 19)),
            (blocky_levels(rng, 15, 19), random_levels(rng, 15, 19))]


def test_identities():
    for a, g in _identity_pairs():
        same = matte_errors_ref(g, g)
        assert (same["sad"], same["sse"], same["conn"], same["grad"]) == (0, 0, 0, 0.0) and same["n"] == g.size
        ab, ba = matte_errors_ref(a, g), matte_errors_ref(g, a)
        assert np.array_equal(ab["levels"], ba["levels"])
        assert all(ab[k] == ba[k] for k in INTS) and ab["grad"] == ba["grad"]
        empty = matte_errors_ref(a, g, np.zeros(a.shape, np.uint8))
        assert (empty["n"], empty["sad"], empty["sse"], empty["conn"], empty["grad"]) == (0, 0, 0, 0, 0.0)
        assert conventional(empty)["mse"] == 0.0
        assert np.array_equal(empty["levels"], ab["levels"])          # the region restricts the sums only


def test_constant_pairs():
    z, o = np.zeros((6, 7), np.uint8), np.full((6, 7), 255, np.uint8)
    e = matte_errors_ref(z, z)
    assert (e["sad"], e["sse"], e["conn"], e["grad"]) == (0, 0, 0, 0.0) and (e["levels"] == 0).all()
    e = matte_errors_ref(o, o)
    assert (e["sad"], e["sse"], e["conn"], e["grad"]) == (0, 0, 0, 0.0) and (e["levels"] == 10).all()
    e = matte_errors_ref(z, o)
    assert (e["n"], e["sad"], e["sse"], e["conn"]) == (42, 42 * 255, 42 * 65025, 42 * 2550) and e["grad"] < 1e-25
    assert (e["levels"] == 0).all()
    c = conventional(e)
    assert c["mse"] == 1.0 and abs(c["sad"] - 0.042) < 1e-15 and abs(c["conn"] - 0.042) < 1e-15


def test_scene_figures_agree_with_the_throwaway_version_of_the_issue():
    """Six significant digits recorded when the feature was proposed, from another restatement of the definition."""
    from closed_form_ref import strand_scene
    from matte_ref import alpha_matte_ref, soft_disk_scene
    want = {("disk", "hard"): (0.186902, 3.22639e-3, 0.115035, 0.189333),
            ("disk", "guided"): (0.035141, 8.30730e-5, 0.008705, 0.004475),
            ("strands", "hard"): (0.287102, 5.45791e-3, 0.386841, 0.290441),
            ("strands", "guided"): (0.124894, 1.58122e-3, 0.199289, 0.091829)}
    for kind, scene in (("disk", soft_disk_scene(seed=0)), ("strands", strand_scene(seed=0))):
        img, alpha, mask = scene
        gt = to_levels(alpha)
        for matte, pred in (("hard", (mask * 255).astype(np.uint8)), ("guided", to_levels(alpha_matte_ref(img, mask, 4, 1e-4)))):
            c = conventional(matte_errors_ref(pred, gt))
            for got, ref in zip((c["sad"], c["mse"], c["grad"], c["conn"]), want[kind, matte]):
                assert abs(got - ref) <= 1e-5 * ref + 5e-7, (kind, matte, got, ref)


# ---------------------------------------------------------------- host side, before any device call
def _no_device(monkeypatch):
    from gcn_grabcut import _engine

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_engine, "get_engine", boom)


@pytest.mark.parametrize("what", ["shape", "above", "below", "nan", "inf", "region", "dtype", "ndim"])
def test_evaluate_matte_refuses_bad_inputs_on_the_host(monkeypatch, what):
    from gcn_grabcut import evaluate_matte
    _no_device(monkeypatch)
    a = np.linspace(0.0, 1.0, 30).reshape(5, 6)
    g = a[::-1].copy()
    region = None
    if what == "shape":
        g = g[:, :5]
    elif what == "above":
        a[2, 2] = 1.0001
    elif what == "below":
        g[0, 0] = -1e-6
    elif what == "nan":
        a[1, 1] = np.nan
    elif what == "inf":
        g[1, 1] = np.inf
    elif what == "region":
        region = np.ones((5, 5), np.uint8)
    elif what == "dtype":
        a = (a * 255).astype(np.int32)
    elif what == "ndim":
        a, g = a[None, None], g[None, None]
    with pytest.raises(ValueError):
        evaluate_matte(a, g, region)


def test_result_without_a_matte_refuses_matte_evaluation(monkeypatch):
    from gcn_grabcut import SegmentationResult
    _no_device(monkeypatch)
    z = np.zeros((4, 5), np.uint8)
    r = SegmentationResult(image=np.zeros((4, 5, 3), np.uint8), binary_mask=z, trimap=z, segments=z.astype(np.int32),
                           overlay=np.zeros((4, 5, 3), np.uint8), rgba=np.zeros((4, 5, 4), np.uint8))
    with pytest.raises(ValueError, match="matte"):
        r.evaluate_matte_against(z)


def test_host_shape_rules():
    from gcn_grabcut._engine import check_matte_eval_args
    check_matte_eval_args((2, 5, 6), (2, 5, 6))
    check_matte_eval_args((0, 5, 6), (0, 5, 6), (0, 5, 6))
    check_matte_eval_args((1, 32768, 32768), (1, 32768, 32768))
    for bad in [((2, 5, 6), (2, 5, 7), None), ((2, 5, 6), (2, 5, 6), (2, 6, 5)), ((5, 6), (5, 6), None),
                ((65536, 1, 1), (65536, 1, 1), None), ((1, 32769, 1), (1, 32769, 1), None), ((1, 0, 4), (1, 0, 4), None),
                ((1, 4, 32769), (1, 4, 32769), None)]:
        with pytest.raises(ValueError):
            check_matte_eval_args(*bad)


def test_scaling_arithmetic_from_raw_sums():
    from gcn_grabcut import MatteMetrics
    from gcn_grabcut.metrics import matte_metrics_from_sums
    m = matte_metrics_from_sums((45, 408, 41616, 4080), 2500.0)
    assert isinstance(m, MatteMetrics)
    assert m.n_pixels == 45 and m.sad == 408 / 255.0 / 1000.0 and m.mse == 41616 / 65025.0 / 45
    assert m.grad == 2.5 and m.conn == 4080 / 2550.0 / 1000.0
    assert m.as_dict() == dict(sad=m.sad, mse=m.mse, grad=m.grad, conn=m.conn, n_pixels=45)
    assert "SAD=0.0016" in str(m) and "Grad=2.5000" in str(m) and "N=45" in str(m)
    e = matte_metrics_from_sums((0, 0, 0, 0), 0.0)
    assert (e.sad, e.mse, e.grad, e.conn, e.n_pixels) == (0.0, 0.0, 0.0, 0.0, 0)
    a, g = tie_case()
    ref = matte_errors_ref(a, g)
    assert matte_metrics_from_sums([ref[k] for k in INTS], ref["grad"]).as_dict() == conventional(ref)


def test_new_names_are_exported_from_both_packages():
    import gcn_grabcut
    import src.gcn_grabcut as shim
    for name in ("evaluate_matte", "evaluate_matte_batch", "MatteMetrics"):
        assert name in gcn_grabcut.__all__ and hasattr(gcn_grabcut, name) and hasattr(shim, name)
    assert hasattr(gcn_grabcut.SegmentationResult, "evaluate_matte_against")


def _cli(*argv):
    return subprocess.run([sys.executable, str(ROOT / "evaluate_matte.py"), *argv], capture_output=True, text=True,
                          timeout=120)


def _write(path, a):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(a).save(path)


def test_cli_refuses_misuse_without_a_traceback(tmp_path):
    a, g = tie_case()
    _write(tmp_path / "gt" / "x.png", g)
    _write(tmp_path / "pred" / "x.png", a)
    _write(tmp_path / "pred2" / "y.png", a)
    _write(tmp_path / "small" / "x.png", a[:, :5].copy())
    gt, pred = str(tmp_path / "gt"), str(tmp_path / "pred")
    cases = [((["--alphas", gt]), "either --pred"),                                          # neither input mode
             (["--alphas", gt, "--pred", pred, "--images", pred, "--masks", pred], "either --pred"),       # both
             (["--alphas", gt, "--images", pred], "go together"),
             (["--alphas", gt, "--pred", str(tmp_path / "pred2")], "no true matte"),
             (["--alphas", gt, "--pred", str(tmp_path / "small")], "is 5x5 but"),
             (["--alphas", gt, "--pred", pred, "--trimaps", str(tmp_path / "pred2")], "no trimap"),
             (["--alphas", gt, "--pred", str(tmp_path / "missing")], "does not exist"),
             (["--alphas", gt, "--images", pred, "--masks", pred, "--method", "guided", "--matte-radius", "65"], "radius"),
             (["--alphas", gt, "--images", pred, "--masks", pred, "--method", "closed-form", "--cf-tol", "2"], "tol")]
    for argv, word in cases:
        r = _cli(*argv)
        assert r.returncode != 0 and word in r.stderr and "Traceback" not in r.stderr, (argv, r.returncode, r.stderr)
