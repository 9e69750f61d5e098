"""The identity behind the warm graph rebuild (csrc/ggc_gc.h, mf_warm_pixel), in numpy and independent of the device code.

A warm build used to re-derive a pixel's terminal balance from the capacities, bal = tw[s] + sum (rc - cap).  The solver
moves one amount in ex and in the two arcs of a link with every push, and lowers ex and snk together when it pushes to the
sink, so any state it leaves satisfies ex - snk = tw[s-1] + sum (rc - cap), and the rebuild is
    bal = (ex - snk) + (tw[s] - tw[s-1])
in the same integers.  Checked here on maximum preflows of the `warm` family (tests/maxflow_nets.py) built from scipy's
maximum_flow, which leave trapped excess, with the definite pixels at the lambda of the family and at the interface's
bound |tw| = 2^27, and on hand-made states at the bounds of both terms, where the int32 arithmetic of the kernel is
compared with int64."""
import numpy as np
import pytest

import maxflow_nets as mn

SHAPES = [(7, 9), (33, 65)]


def _chain(h, w, lam):
    tw, nw = mn.make("warm", "resample", h, w, seed=4)
    tw = tw.astype(np.int64)
    if lam != 30000:                                       # the family pins its definite pixels at +-30000
        tw = np.where(np.abs(tw) == 30000, np.sign(tw) * lam, tw)
    return tw.astype(np.int32), nw


def _kernel_i32(ex, snk, tw_new, tw_old):
    """mf_warm_pixel in int32, as the device computes it (numpy wraps silently, so a wrap would show as a mismatch)."""
    with np.errstate(over="ignore"):
        bal = (ex.astype(np.int32) - snk.astype(np.int32)) + (tw_new.astype(np.int32) - tw_old.astype(np.int32))
    return np.maximum(bal, 0), np.maximum(-bal, 0)


@pytest.mark.parametrize("lam", [30000, mn.TW_MAX])
@pytest.mark.parametrize("h,w", SHAPES)
def test_balance_identity_on_maximum_preflows(h, w, lam):
    tw, nw = _chain(h, w, lam)
    assert np.abs(tw).max() == lam
    cap = mn._arc_caps(nw)
    trapped = 0
    for s in range(1, tw.shape[0]):
        res, _ = mn.state_from_scipy(tw[s - 1], nw)
        rc, ex, snk = res[:, :, :8], res[:, :, 8], res[:, :, 9]
        trapped += int((ex > 0).sum())
        inflow = (rc - cap).sum(axis=2)
        old = tw[s].astype(np.int64) + inflow                                   # what the build used to compute
        new = (ex - snk) + (tw[s].astype(np.int64) - tw[s - 1].astype(np.int64))
        assert np.array_equal(new, old), (s, np.argwhere(new != old)[:4].tolist())
        e32, k32 = _kernel_i32(ex, snk, tw[s], tw[s - 1])
        assert np.array_equal(e32, np.maximum(old, 0)) and np.array_equal(k32, np.maximum(-old, 0)), s
        # the rebuilt state is a valid preflow of step s on the old capacities: the balance of certify() holds again
        assert np.array_equal(e32.astype(np.int64) - k32, tw[s] + inflow)
        assert (np.minimum(e32, k32) == 0).all()
    assert trapped > 0, "no state of the chain holds trapped excess"


def test_identity_survives_every_kind_of_push():
    """Random pushes (to a neighbour, to the sink) from the initial preflow keep ex - snk = tw + sum (rc - cap)."""
    tw, nw = mn.make("warm", "resample", 7, 9, seed=9)
    tw0 = tw[0].astype(np.int64)
    cap = mn._arc_caps(nw)
    rc, ex, snk = cap.copy(), np.maximum(tw0, 0), np.maximum(-tw0, 0)
    rng = np.random.default_rng(0)
    h, w = tw0.shape
    both = False
    for _ in range(4000):
        both |= bool(((ex > 0) & (snk > 0)).any())
        y, x = int(rng.integers(h)), int(rng.integers(w))
        if ex[y, x] == 0:
            continue
        if snk[y, x] > 0 and rng.random() < 0.5:
            dl = min(ex[y, x], snk[y, x]); ex[y, x] -= dl; snk[y, x] -= dl
            continue
        d = int(rng.integers(8))
        dy, dx = mn.DIRS[d][:2]
        if not (0 <= y + dy < h and 0 <= x + dx < w) or rc[y, x, d] == 0:
            continue
        dl = min(ex[y, x], rc[y, x, d])
        rc[y, x, d] -= dl; rc[y + dy, x + dx, d ^ 1] += dl
        ex[y, x] -= dl; ex[y + dy, x + dx] += dl
    assert (rc != cap).any() and both                               # mid-solve pixels held excess and sink capacity at once
    assert np.array_equal(ex - snk, tw0 + (rc - cap).sum(axis=2))
    e32, k32 = _kernel_i32(ex, snk, tw[1], tw[0])
    want = tw[1].astype(np.int64) + (rc - cap).sum(axis=2)
    assert np.array_equal(e32, np.maximum(want, 0)) and np.array_equal(k32, np.maximum(-want, 0))


def test_int32_holds_at_the_bounds():
    """|ex - snk| <= 2^27 + 8 * 2^24 = 2^28 (all eight links of a pixel at 2^24 carrying flow one way), |tw - tw_old| <= 2^28:
    the sum stays within 2^29."""
    t, n8 = mn.TW_MAX, 8 * mn.NW_MAX
    ex = np.array([t + n8, 0, t + n8, 0, 0], np.int64)
    snk = np.array([0, t + n8, 0, t + n8, 0], np.int64)
    tw_old = np.array([t, -t, -t, t, 0], np.int64)
    tw_new = np.array([-t, t, t, -t, t], np.int64)
    want = (ex - snk) + (tw_new - tw_old)
    assert np.abs(want).max() == 3 * t + n8 and 3 * t + n8 <= 1 << 29
    e32, k32 = _kernel_i32(ex, snk, tw_new, tw_old)
    assert np.array_equal(e32, np.maximum(want, 0)) and np.array_equal(k32, np.maximum(-want, 0))
