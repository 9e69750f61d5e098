"""Foreground colour estimation without a GPU: the float64 restatement (tests/foreground_ref.py) against a dense direct
solve, the quality and agreement margins the GPU test holds the device to, and the host-side argument checks of the
engine, the pipeline and the command line."""
import numpy as np
import pytest

from foreground_ref import (ALPHA_SOURCES, DELTA, System, alpha_input, dense_matrix, dense_solve, pcg, premult_levels,
                            quality_ratio, residual_norms, scene_colours, snap)
from matte_ref import edge_band

DEFAULTS = dict(eps_r=5e-3, omega=1.0, max_iter=2000, tol=1e-6)     # pipeline.FG_* (checked below)
SCENES = (("disk", 0), ("disk", 1), ("strands", 0))
# error(alpha', clamp F) / error(alpha, I) on edge_band(mask, 8), per alpha source.  Restatement, at the defaults:
# true 0.081 0.080 0.067; closed-form matte 0.154 0.191 0.361; guided matte 0.322 0.292 0.538 (disk0, disk1, strands0)
QUALITY = {"true": 0.15, "closed": 0.5, "guided": 0.7}
AGREE_LEVELS = 0.5     # device at the default tol vs the restatement at 1e-12, premultiplied colours, in byte levels
AGREE_LEVELS_CPU = 0.1  # the same between two runs of the restatement (measured: at most 0.074 and 0.087)


def _noise_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def _tiny_cases():
    rng = np.random.default_rng(5)
    h, w = 7, 9
    a = rng.random((h, w))
    a[rng.random((h, w)) < 0.25] = 0.0
    a[rng.random((h, w)) < 0.25] = 1.0
    yield "random", _noise_image(h, w, 1), a
    yield "empty", _noise_image(h, w, 2), (rng.random((h, w)) < 0.5).astype(np.float64)
    yield "constant", _noise_image(h, w, 3), np.full((h, w), 0.5)          # no Dirichlet value: the case delta exists for
    one = np.zeros((h, w))
    one[3, 4] = 0.3
    yield "one-pixel", _noise_image(h, w, 4), one
    only_z = np.zeros((h, w))
    only_z[2:5, 3:7] = rng.uniform(0.1, 0.9, (3, 4))
    yield "touches-only-Z", _noise_image(h, w, 6), only_z
    only_o = np.ones((6, 5))
    only_o[1:4, 1:4] = rng.uniform(0.1, 0.9, (3, 3))
    yield "touches-only-O", _noise_image(6, 5, 7), only_o


@pytest.mark.parametrize("name,img,alpha", list(_tiny_cases()), ids=[c[0] for c in _tiny_cases()])
@pytest.mark.parametrize("eps_r,omega", [(5e-3, 1.0), (1e-2, 0.0), (0.0, 0.5)])
def test_pcg_matches_a_dense_solve(name, img, alpha, eps_r, omega):
    # the smallest eigenvalue of A is at least delta = 1e-6 and the largest of order 1, so a relative residual of 1e-12
    # bounds the error by about 1e-6; the raw bound allows 10x for ||r_0|| above 1
    a = snap(alpha)
    F, B, it, rel = pcg(img, a, eps_r, omega, 20000, 1e-12)
    wF, wB = dense_solve(img, a, eps_r, omega)
    U = (a > 0) & (a < 1)
    assert np.array_equal(F[~U], img[~U] / 255.0) and np.array_equal(B[~U], img[~U] / 255.0)
    if name == "empty":
        assert it == 0 and rel == 0.0 and not U.any()
    elif name == "constant" and eps_r == 0.0:                   # every link weight is 0: F = B = I solves each pixel
        assert it == 0 and rel == 0.0
    else:
        _, r0 = residual_norms(img, a, eps_r, omega, F, B)      # on so few pixels the absolute floor can be the active term
        assert it >= 1 and rel <= max(1e-12, 1e-12 * np.sqrt(6.0 * U.sum()) / r0)
    assert np.abs(F - wF).max() <= 1e-5 and np.abs(B - wB).max() <= 1e-5
    assert np.abs(a[..., None] * (F - wF)).max() <= 1e-6 and np.abs((1 - a[..., None]) * (B - wB)).max() <= 1e-6


def test_system_is_symmetric_positive_definite_and_is_the_energy():
    rng = np.random.default_rng(11)
    img = _noise_image(9, 11, 8)
    a = snap(rng.random((9, 11)) * 1.4 - 0.2)
    for eps_r, omega in ((5e-3, 1.0), (0.0, 1.0)):
        A, b, s = dense_matrix(img, a, eps_r, omega)
        assert np.abs(A - A.T).max() <= 1e-15
        assert np.linalg.eigvalsh(A).min() >= DELTA
        # E(x) = x^T A x - 2 b^T x + c: check on two random points against the energy written out
        n = len(b) // 2
        es = []
        for _ in range(3):
            x = rng.standard_normal(2 * n)
            F, B = s.I.copy(), s.I.copy()
            F[s.U], B[s.U] = x[:n].reshape(-1, 3), x[n:].reshape(-1, 3)
            es.append(s.energy(F, B) - (x @ A @ x - 2.0 * b @ x))
        assert max(es) - min(es) <= 1e-9 * max(1.0, abs(es[0]))


def test_flat_image_and_solved_start_take_no_iterations():
    rng = np.random.default_rng(3)
    a = snap(rng.random((20, 24)))
    img = np.full((20, 24, 3), 90, np.uint8)
    F, B, it, rel = pcg(img, a, 5e-3, 1.0, 100, 1e-6)
    assert it == 0 and rel == 0.0 and np.array_equal(F, img / 255.0)


def test_snap_follows_the_alpha_byte():
    a = np.array([-1.0, 0.0, 1 / 510 - 1e-9, 1 / 510, 0.5, 1 - 1 / 510, 1 - 1 / 510 + 1e-9, 1.0, 2.0, np.nan, np.inf, -np.inf])
    assert np.array_equal(snap(a), [0, 0, 0, 1 / 510, 0.5, 1 - 1 / 510, 1, 1, 1, 0, 1, 0])
    x = np.linspace(0, 1, 100001)
    byte = np.floor(255 * x + 0.5)
    s = snap(x)
    assert np.array_equal(s == 0, byte == 0) and np.array_equal(s == 1, byte == 255)


@pytest.mark.parametrize("kind,seed", SCENES)
def test_scene_colours_replays_the_scene(kind, seed):
    img, a, m, fg, bg = scene_colours(kind, seed)
    assert img.shape == (120, 160, 3) and fg.shape == bg.shape == (120, 160, 3)
    assert 150 <= fg.min() and fg.max() <= 250 and 10 <= bg.min() and bg.max() <= 110
    frac = (a > 0.1) & (a < 1)
    assert 55 <= np.abs(img - fg)[frac].mean() <= 75            # the colour bleed a cut-out of image bytes carries


@pytest.mark.parametrize("source", ALPHA_SOURCES)
@pytest.mark.parametrize("kind,seed", SCENES)
def test_restatement_meets_the_quality_and_agreement_margins(kind, seed, source):
    img, a_true, mask, fg, _ = scene_colours(kind, seed)
    alpha = alpha_input(kind, seed, source)
    d = DEFAULTS
    s = snap(alpha)
    F, B, it, rel = pcg(img, s, d["eps_r"], d["omega"], d["max_iter"], d["tol"])
    assert 1 <= it < d["max_iter"] and rel <= d["tol"]
    ratio = quality_ratio(alpha, F, img, a_true, fg, edge_band(mask, 8))
    F2, B2, _, rel2 = pcg(img, s, d["eps_r"], d["omega"], 20000, 1e-12)
    assert rel2 <= max(1e-12, 1e-12 * np.sqrt(6.0 * ((s > 0) & (s < 1)).sum()) / residual_norms(img, s, d["eps_r"], d["omega"], F, B)[1])
    pf, pb = premult_levels(s, F, B)
    qf, qb = premult_levels(s, F2, B2)
    df, db = np.abs(pf - qf).max(), np.abs(pb - qb).max()
    res, res0 = residual_norms(img, s, d["eps_r"], d["omega"], F, B)
    print(f"{kind}{seed} {source}: iterations {it}, ratio {ratio:.3f}, premultiplied F {df:.3f} B {db:.3f} levels, "
          f"residual {res / res0:.3e} (recurrence {rel:.3e})")
    assert ratio <= QUALITY[source]
    assert df <= AGREE_LEVELS_CPU and db <= AGREE_LEVELS_CPU
    assert abs(res / res0 - rel) <= 0.1 * rel


# ---------------------------------------------------------------- host side, before any device call
def test_defaults_are_the_recorded_choice():
    from gcn_grabcut import ForegroundColours
    from gcn_grabcut import pipeline as P
    c = ForegroundColours()
    assert c.args() == (DEFAULTS["eps_r"], DEFAULTS["omega"], DEFAULTS["max_iter"], DEFAULTS["tol"])
    assert (P.FG_EPS_R, P.FG_OMEGA, P.FG_MAX_ITER, P.FG_TOL) == c.args()
    with pytest.raises(Exception):
        c.omega = 2.0                                            # frozen


BAD_ARGS = [(-1e-3, 1.0, 10, 1e-6), (1.5, 1.0, 10, 1e-6), (float("nan"), 1.0, 10, 1e-6), (5e-3, -1.0, 10, 1e-6),
            (5e-3, 1001.0, 10, 1e-6), (5e-3, float("inf"), 10, 1e-6), (0.0, 0.0, 10, 1e-6), (5e-3, 1.0, 0, 1e-6),
            (5e-3, 1.0, 100001, 1e-6), (5e-3, 1.0, 2.5, 1e-6), (5e-3, 1.0, 10, 0.0), (5e-3, 1.0, 10, 1.0),
            (5e-3, 1.0, 10, float("nan"))]


@pytest.mark.parametrize("args", BAD_ARGS)
def test_host_refuses_bad_foreground_arguments(args):
    from gcn_grabcut import estimate_foreground
    from gcn_grabcut._engine import check_foreground_args
    with pytest.raises(ValueError):
        check_foreground_args(*args)
    img = _noise_image(12, 12, 0)
    with pytest.raises(ValueError):
        estimate_foreground(img, np.full((12, 12), 0.5, np.float32), *args)


def test_host_accepts_the_edges_of_the_range():
    from gcn_grabcut._engine import check_foreground_args
    for args in ((0.0, 1.0, 1, 1e-12), (1.0, 0.0, 100000, 0.999), (5e-3, 1000.0, 2000, 1e-6)):
        check_foreground_args(*args)


def test_public_estimate_foreground_refuses_bad_alpha_before_any_device_call():
    from gcn_grabcut import estimate_foreground
    img = _noise_image(12, 12, 1)
    with pytest.raises(ValueError, match="does not match"):
        estimate_foreground(img, np.zeros((12, 11), np.float32))
    with pytest.raises(ValueError, match="float"):
        estimate_foreground(img, np.zeros((12, 12), np.uint8))


def test_pipeline_routes_the_foreground_arguments():
    from gcn_grabcut import ClosedFormMatte, ForegroundColours
    from gcn_grabcut.pipeline import _foreground_args
    assert _foreground_args(False, True, False) is None and _foreground_args(None, False, True) is None
    assert _foreground_args(True, True, False) == (5e-3, 1.0, 2000, 1e-6)
    assert _foreground_args(ForegroundColours(omega=0.5, tol=1e-4), ClosedFormMatte(), False) == (5e-3, 0.5, 2000, 1e-4)
    with pytest.raises(ValueError, match="matte"):
        _foreground_args(True, False, False)
    with pytest.raises(ValueError, match="full"):
        _foreground_args(True, True, True)
    with pytest.raises(ValueError):
        _foreground_args(ForegroundColours(eps_r=0.0, omega=0.0), True, False)
    with pytest.raises(ValueError):
        _foreground_args("yes", True, False)


def test_pipeline_refuses_foreground_without_a_matte_or_with_a_full_image_before_any_stage():
    # no stage may run: the pipeline object is built without a device and every stage entry raises if reached
    from gcn_grabcut import ClosedFormMatte, GCNGrabCutPipeline
    pipe = GCNGrabCutPipeline.__new__(GCNGrabCutPipeline)

    def stage(*a, **k):
        raise AssertionError("a stage ran")

    class NoEngine:
        def __getattr__(self, name):
            return stage

    pipe._eng = NoEngine()
    img = _noise_image(40, 50, 3)
    for call in (lambda: pipe.segment(img, foreground=True),
                 lambda: pipe.segment_bbox(img, (5, 5, 30, 20), foreground=True),
                 lambda: pipe.segment_batch([img, img], foreground=True)):
        with pytest.raises(ValueError, match="matte"):
            call()
    for call in (lambda: pipe.segment(img, matte=True, foreground=True, full_image=img),
                 lambda: pipe.segment_bbox(img, (5, 5, 30, 20), matte=True, foreground=True, full_image=img),
                 lambda: pipe.segment_batch([img, img], matte=True, foreground=True, full_images=[img, img])):
        with pytest.raises(ValueError, match="full"):
            call()


def test_cli_offers_decontaminate():
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import inference
    p = inference.build_parser()
    d = p.parse_args(["--image", "x.png"])
    assert d.decontaminate is False
    assert (d.decon_eps, d.decon_omega, d.decon_iters, d.decon_tol) == (5e-3, 1.0, 2000, 1e-6)
    a = p.parse_args(["--image", "x.png", "--save", "cutout", "--decontaminate", "--decon-eps", "1e-3", "--decon-omega",
                      "0.5", "--decon-iters", "300", "--decon-tol", "1e-4", "--fg-point", "3,4"])
    assert a.decontaminate and (a.decon_eps, a.decon_omega, a.decon_iters, a.decon_tol) == (1e-3, 0.5, 300, 1e-4)
    assert a.fg_point == [(3, 4)]
    help_text = p.format_help()
    for flag in ("--decontaminate", "--decon-eps", "--decon-omega", "--decon-iters", "--decon-tol"):
        assert flag in help_text


@pytest.mark.parametrize("extra,word", [(["--full-res", "--save", "cutout"], "full-res"), (["--save", "alpha"], "cutout"),
                                        (["--save", "cutout", "--decon-tol", "2"], "tol")])
def test_cli_refuses_decontaminate_misuse(tmp_path, extra, word):
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(root / "inference.py"), "--image", str(tmp_path / "x.png"), "--decontaminate",
                        *extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and word in r.stderr
