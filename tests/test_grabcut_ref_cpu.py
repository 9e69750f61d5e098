"""The oracle's GrabCut, one iteration at a time, against the float64 GrabCut of tests/grabcut_ref.py (no GPU).

The device is bit-exact against the oracle (test_grabcut_gpu.py), so what the oracle gets wrong here the device gets
wrong too.  Each family of grabcut_ref.FAMILIES aims at one mechanism and first asserts that it reaches it."""
import math

import numpy as np
import pytest

import grabcut_ref as gr

N_STEPS = 3


def _ulps(got, want):
    g = np.asarray(got, np.float64).view(np.int64).astype(object)
    w = np.asarray(want, np.float64).view(np.int64).astype(object)
    return np.array([abs(a - b) for a, b in zip(g, w)])


def test_exp_within_2ulp_of_libm_down_to_the_subnormals(oracle):
    L = oracle.lib()
    xs = np.concatenate([np.linspace(-745.2, 709.7, 60001), np.linspace(-745.2, -700.0, 20001),
                         np.linspace(709.0, 709.78, 2001), [-745.13321910194122, -745.1332191019411, -708.4, 0.0]])
    got = np.array([L.ggo_exp(float(x)) for x in xs])
    want = np.array([math.exp(x) for x in xs])
    u = _ulps(got, want)
    assert u.max() <= 2, (xs[u.argmax()], got[u.argmax()], want[u.argmax()])
    assert (got[want == 0.0] == 0.0).all()
    assert L.ggo_exp(-712.0) > 0 and L.ggo_exp(-745.0) == 5e-324       # the band the old -708 flush returned 0 for
    assert L.ggo_exp(-746.0) == 0.0 and L.ggo_exp(709.79) == math.inf and math.isnan(L.ggo_exp(math.nan))


def test_log_within_2ulp_of_libm_subnormals_included(oracle):
    L = oracle.lib()
    lo, hi = np.array([5e-324, 1.8e308]).view(np.int64)
    bits = np.unique(np.concatenate([np.linspace(lo, hi, 60001).astype(np.int64), np.arange(1, 2001, dtype=np.int64),
                                     np.array([2.2250738585072014e-308, 1e-310, 1e-320]).view(np.int64)]))
    xs = bits.view(np.float64)
    got = np.array([L.ggo_log(float(x)) for x in xs])
    want = np.array([math.log(x) for x in xs])
    u = _ulps(got, want)
    assert u.max() <= 2, (xs[u.argmax()], got[u.argmax()], want[u.argmax()])
    assert L.ggo_log(0.0) == -math.inf and math.isnan(L.ggo_log(-1.0))
    assert L.ggo_log(1e-310) == pytest.approx(-713.8, abs=0.05)


def _chain(oracle, st, seed=3, n=N_STEPS):
    """[(mask, bgd, fgd)] for k = 0..n: the start state, then one oracle call (mode 2, n_iter 1) per iteration."""
    s = gr.start(oracle, st, seed)
    assert s is not None, "start state is degenerate"
    out = [s]
    for _ in range(n):
        m, b, f = out[-1]
        _, m1, b1, f1, rc = oracle.grabcut(st["img"], m, n_iter=1, mode=2, bgd=b, fgd=f)
        assert rc == 0
        out.append((m1, b1, f1))
    return out


@pytest.mark.parametrize("family,variant", gr.cases())
def test_oracle_iterations_certified_by_the_reference(oracle, family, variant):
    st = gr.make(family, variant, seed=3)
    states = _chain(oracle, st)
    for k in range(1, len(states)):
        gr.certify_step(oracle, st["img"], *states[k - 1], *states[k], what=f"{family}/{variant} it{k}",
                        exact_ties=st["exact_ties"])


def test_oracle_n_iter_equals_chained_single_iterations(oracle):
    st = gr.make("singular", "few_colours", seed=3)
    states = _chain(oracle, st)
    _, m, b, f, rc = oracle.grabcut(st["img"], st["mask"], n_iter=N_STEPS, mode=0, seed=3)
    assert rc == 0
    assert np.array_equal(m, states[-1][0]) and np.array_equal(b, states[-1][1]) and np.array_equal(f, states[-1][2])


# ------------------------------------------------------------------ each family reaches its mechanism

def test_underflow_family_reaches_the_band(oracle):
    flush = -708.0
    for variant in ("one_side", "both_sides", "assign_flush"):
        st = gr.make("underflow", variant)
        m, b, f = gr.start(oracle, st)
        ref = gr.step(st["img"], m, b, f)
        old = gr.step(st["img"], m, b, f, flush_below=flush)
        band = gr.band_pixels(st["img"], m, ref["bgd"], ref["fgd"])
        assert band.sum() >= 2, variant
        if variant == "one_side":                     # libm: a finite t-link the n-links beat; flushed: +lambda
            assert (np.abs(ref["twf"][band]) < 300).all() and (old["twf"][band] == gr.LAMBDA).all()
            _, cut = oracle.grid_maxflow(ref["tw"], ref["nw"])
            _, cut_old = oracle.grid_maxflow(old["tw"], old["nw"])
            assert (cut[band] == 0).all() and (cut_old[band] == 1).all()
        elif variant == "both_sides":                 # both totals flush: inf - inf -> 0, libm keeps a finite difference
            px = st["img"][band]
            for model in (ref["bgd"], ref["fgd"]):
                mx = gr.scores(model, px)[1].max(1)
                assert ((mx > -745.2) & (mx < flush)).all()
            assert (old["twf"][band] == 0.0).all() and (np.abs(ref["twf"][band]) > 5).all()
        else:                                         # every candidate component flushes: component 0 instead of the argmax
            assert (old["comp"][band] == 0).all() and (ref["comp"][band] == 1).all()
            assert not np.array_equal(old["fgd"], ref["fgd"])


def test_tie_family_breaks_exact_ties_to_the_lowest_index(oracle):
    for variant in ("mirrored", "axis"):
        st = gr.make("ties", variant)
        m, b, f = gr.start(oracle, st)
        px = st["img"].reshape(-1, 3)[(m == gr.GC_PR_BGD).ravel()]
        s, _ = gr.scores(b, px)
        assert (s[:, 0] == s[:, 1]).sum() > 100 and (s[:, 0] > 0).all()     # equal to the last bit
        comp, tie = gr.assign(st["img"], m, b, f)
        assert (comp[m == gr.GC_PR_BGD] == 0).all() and tie.sum() > 100


def test_beta_shape_rect_and_lambda_families_reach_their_edges(oracle):
    assert gr.beta(gr.make("beta", "zero_contrast")["img"]) == 0.0
    assert gr.nlinks(gr.make("beta", "zero_contrast")["img"]).max() == gr.GAMMA
    chk = gr.make("beta", "max_contrast")["img"]
    nw = gr.nlinks(chk)                               # straight pairs always differ, diagonal pairs never by 255
    assert 0 < gr.beta(chk) < 1e-5 and nw[0].max() < nw[1][1:, 1:].min() and nw[2].max() < nw[3][1:, :-1].min()
    for variant, shape in (("1x1", (1, 1)), ("1xN", (1, 97)), ("Nx1", (83, 1)), ("2x2", (2, 2))):
        img = gr.make("shapes", variant)["img"]
        assert img.shape[:2] == shape
        h, w = shape
        assert int(gr.nlinks(img).astype(bool).sum()) <= gr.n_links(h, w)
    for variant in ("leave", "negative"):
        st = gr.make("rect", variant)
        h, w = st["img"].shape[:2]
        x, y, rw, rh = st["rect"]
        assert x < 0 or y < 0 or x + rw > w or y + rh > h
    st = gr.make("near_lambda", "sweep")
    m, b, f = gr.start(oracle, st)
    ref = gr.step(st["img"], m, b, f)
    src, snk = gr.tlinks(st["img"], m, ref["bgd"], ref["fgd"])
    d = np.abs(src - snk)[gr.probable(m)]
    for lo, hi in ((gr.LAMBDA - 10, gr.LAMBDA), (gr.LAMBDA, gr.LAMBDA + 10)):
        assert ((d > lo) & (d < hi)).sum() >= 4, (lo, hi, np.sort(d))


def test_certificate_rejects_a_wrong_mask_and_wrong_models(oracle):
    st = gr.make("singular", "few_colours", seed=3)
    (m0, b0, f0), (m1, b1, f1) = _chain(oracle, st, n=1)
    pr = np.argwhere(gr.probable(m0))
    bad = m1.copy()
    y, x = pr[len(pr) // 2]
    bad[y, x] = gr.GC_PR_BGD if bad[y, x] == gr.GC_PR_FGD else gr.GC_PR_FGD
    with pytest.raises(AssertionError):
        gr.certify_step(oracle, st["img"], m0, b0, f0, bad, b1, f1)
    worse = f1.copy()
    worse[0] *= 1.0 + 1e-9
    with pytest.raises(AssertionError):
        gr.certify_step(oracle, st["img"], m0, b0, f0, m1, b1, worse)
