"""CPU tests of the adversarial max-flow networks (tests/maxflow_nets.py): the oracle's flow value and canonical cut against
scipy's maximum_flow on every family, and the certificate the GPU tests apply to the device's final state — it accepts a
maximum preflow built from scipy's flow and rejects each single corruption of it."""
import numpy as np
import pytest

import maxflow_nets as mn
from test_grabcut_oracle import scipy_cut

SMALL = [(1, 1), (1, 9), (9, 1), (3, 3), (7, 9), (8, 33), (17, 40)]
CASES = [(f, v) for f in mn.VARIANTS for v in mn.VARIANTS[f]]


def _shapes(family):
    if family == "extremes":
        return [(1, 1), (2, 3), (3, 3), (1, 5)]          # scipy's flow value is int32: keep the total flow below 2^31
    if family == "serpentine":
        return [(1, 9), (5, 7), (9, 40), (17, 33)]
    return SMALL


@pytest.mark.parametrize("family,variant", CASES)
def test_oracle_matches_scipy_on_every_family(oracle, family, variant):
    for h, w in _shapes(family):
        tw, nw = mn.make(family, variant, h, w, seed=1)
        nz = mn._zero_outside(nw)                          # scipy_cut would read out-of-image planes; the oracle ignores them
        for s in range(tw.shape[0]):
            flow, side = oracle.grid_maxflow(tw[s], nw)
            want_flow, want_side = scipy_cut(tw[s], nz)
            assert flow == want_flow, (family, variant, h, w, s)
            assert np.array_equal(side, want_side), (family, variant, h, w, s)


def test_families_hit_their_targets():
    tw, nw = mn.make("serpentine", "mid_bottleneck", 96, 128)
    assert (nw > 0).sum() == 48 * 128 + 47 - 1             # one corridor: 48 rows and 47 connectors, one link per step
    tw, nw = mn.make("corner_gates", "gates", 64, 96)
    for k, (dy, dx) in enumerate(mn.PLANE_OFF):
        ys, xs = np.nonzero(nw[k])
        crosses_x = (xs + dx) // 32 != xs // 32
        crosses_y = (ys + dy) // 8 != ys // 8
        assert not (crosses_x ^ crosses_y).any()           # a border is crossed only at a corner
        if k in (1, 3):
            assert (crosses_x & crosses_y).any()
    tw, nw = mn.make("extremes", "checker", 8, 8)
    assert np.abs(tw).max() == mn.TW_MAX and nw.max() == mn.NW_MAX
    tw, nw = mn.make("warm", "resample", 40, 50)
    assert tw.shape[0] == 4
    for s in range(1, 4):
        changed = tw[s] != tw[s - 1]
        assert 0.1 < changed.mean() < 0.3 and (np.sign(tw[s][changed]) != np.sign(tw[s - 1][changed])).mean() > 0.9


@pytest.mark.parametrize("family,variant", [("random", "dense"), ("serpentine", "mid_bottleneck"), ("corner_gates", "gates"),
                                            ("border_bottlenecks", "tiles_32x8"), ("extremes", "one_sink"),
                                            ("degenerate", "outside_garbage"), ("warm", "resample")])
def test_certificate_accepts_scipys_maximum_flow(oracle, family, variant):
    h, w = (3, 3) if family == "extremes" else (17, 40)
    tw, nw = mn.make(family, variant, h, w, seed=2)
    for s in range(tw.shape[0]):
        res, value = mn.state_from_scipy(tw[s], nw)
        flow, side = oracle.grid_maxflow(tw[s], nw)
        assert value == flow
        mn.certify(tw[s], nw, side, res, flow, cold=True)


def _corrupt(kind, tw, nw, side, res, flow):
    res, side = res.copy(), side.copy()
    h, w = tw.shape
    c = mn._arc_caps(nw)
    if kind == "arc_below_zero":                           # an empty arc at -1, its partner one up: only check 1 can see it
        y, x, d = np.argwhere((res[:, :, :8] == 0) & (c > 0))[0]
        dy, dx = mn.DIRS[d][:2]
        res[y, x, d] -= 1
        res[y + dy, x + dx, d ^ 1] += 1
        return res, side, flow, "negative residual"
    if kind == "arc_plus_one":
        y, x, d = np.argwhere(c > 0)[3]
        res[y, x, d] += 1
        return res, side, flow, "pair sum"
    if kind == "excess_plus_one":
        y, x = np.argwhere(res[:, :, 8] > 0)[0]
        res[y, x, 8] += 1
        return res, side, flow, "balance"
    if kind == "pixel_across_cut":
        y, x = np.argwhere(side == 0)[0]
        side[y, x] = 1
        return res, side, flow, "source_side"
    if kind == "trapped_excess_on_sink_side":
        y, x = np.argwhere((res[:, :, 8] > 0) & (side == 1))[0]
        side[y, x] = 0
        return res, side, flow, "source_side"
    if kind == "wrong_flow_value":
        return res, side, flow + 1, "cut capacity"
    if kind == "nothing_pushed":                           # the initial preflow: valid, canonical labels, but not maximal
        res[:, :, :8] = c
        res[:, :, 8] = np.maximum(tw, 0)
        res[:, :, 9] = np.maximum(-tw, 0)
        side = (~mn.reaches_sink(res[:, :, :8], res[:, :, 9])).astype(np.uint8)
        return res, side, flow, "not maximal"
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["arc_below_zero", "arc_plus_one", "excess_plus_one", "pixel_across_cut",
                                  "trapped_excess_on_sink_side", "wrong_flow_value", "nothing_pushed"])
def test_certificate_rejects_a_single_corruption(oracle, kind):
    tw, nw = mn.make("border_bottlenecks", "tiles_32x8", 24, 70, seed=3)
    tw = tw[0]
    res, flow = mn.state_from_scipy(tw, nw)
    _, side = oracle.grid_maxflow(tw, nw)
    mn.certify(tw, nw, side, res, flow, cold=True)         # the uncorrupted state passes
    bad_res, bad_side, bad_flow, what = _corrupt(kind, tw, nw, side, res, flow)
    with pytest.raises(AssertionError, match=what):
        mn.certify(tw, nw, bad_side, bad_res, bad_flow, cold=True)
