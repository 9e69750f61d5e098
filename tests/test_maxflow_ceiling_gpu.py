"""The label ceiling of the max-flow's push phases (GGC_MF_LABEL_SLACK; csrc/ggc_mf_push.h).

After a round's relabel the active scan leaves lmax[b], the largest finite label of image b.  During that round's push phase a
pixel whose label reaches lim = min(H * W, lmax + 1 + slack) keeps its excess and waits for the next global relabel, as a pixel
at label H * W always did.  Right after a relabel nothing holds label lmax + 1, so everything above is cut off from the sink;
where local relabels have filled that level since, the ceiling parks excess that could still have moved.  That may cost a
round and never the result: an image is closed only by the active scan after an exact relabel, on `label < infinity`.

The library reads its GGC_MF_* switches once per process, so each setting runs in one child interpreter (one at a time, with a
time limit).  Every network goes through ggc_grid_maxflow (tests/maxflow_nets.py): every step's cut must equal the CPU
oracle's and the final state must pass the max-flow/min-cut certificate.  The oracle's cuts are computed once, in this
process, and handed to the children in a file.

1. test_ceiling_matches_oracle_and_certifies: the families of maxflow_nets (random, serpentine, corner gates, both
   border-bottleneck variants, capacities at the bounds, the warm family, the batch of five with its closed all_sink image) at
   1x1 .. 96x128 with slack 0, a slack of 4, the library's default (slack 0, here without the variable set) and the ceiling
   off, each under the default schedule, the all-asynchronous one and the all-dense one.

2. test_detour_is_parked_and_released: the smallest network on which the ceiling is WRONG.  One 8x32 tile; a source S of 100
   at the left end of a corridor along row 3 (links of 1000), a sink T1 right above S behind a link of 5, a sink T2 at the
   corridor's right end, 31 links away.  The relabel labels the corridor from both ends (T2 from the right, T1 through S from
   the left), so lmax = 17 is the ridge in its middle.  S sends 5 to T1, the link saturates, and the remaining 95 must climb
   the left slope: whoever holds them next to the ridge needs label 18 = lmax + 1 to get across and is parked there at slack 0,
   although T2 is reachable.  The next exact relabel finds the corridor's labels falling from S (32) to T2, the excess runs
   down, and a third round finds nothing active.  Without the ceiling the excess crosses the ridge within the first visit: two
   rounds.  Every round is one dense launch, one visit of the tile, with as many sweeps as it takes, and exact relabels
   (GGC_MF_PARTIAL_ROUNDS=0).  _simulate() below restates that schedule in numpy (exact relabel; per sweep one synchronous
   push-or-relabel step of every active pixel by the visit's rule: the sink link first, else the lowest-labelled residual
   neighbour, first direction on ties) and gives 3 rounds with the ceiling, 2 without, and the sweeps a visit needs; the test
   gives a visit four times the simulated sweeps.  The device's lanes push one after another where the simulation steps them
   together, but the excess here is ONE unit that moves as a whole, so the device may not need more rounds than simulated:
   the bound is the simulated count itself, and the count without the ceiling is recorded beside it.  The trace's count of
   parked excess that the relabel found reachable must be non-zero in the ceiling run and zero without.

3. test_sealed_pocket_retires_below_the_ceiling: a pocket of 8 x 18 pixels across the border of the two tiles of an 8x64 image,
   every pixel holding 5, wide links inside, and ONE exit link of 40 to an open region three pixels deep that ends in sinks;
   everything else is isolated.  The dense first round is cut down to one sweep, so the exit saturates inside the
   asynchronous launch of round 1 (chains of up to 127 hops): from then on the pocket's excess is handed back and forth and its
   labels climb, to lim = lmax + 1 (about 25) with the ceiling and towards H * W = 512 without.  With the ceiling every chain
   must end with nothing to hand on (none cut by the hop limit), and the solve's asynchronous visits must stay below the
   ceiling-off run of the same library by the margin of the restatement: _simulate() counts the sweeps of round 1 until
   nothing is active, s_lim and s_off (the latter capped by the chain budget of 127 hops x 12 sweeps); visits are sweeps / 12
   per tile in either run, so the ratio of visits is the ratio of sweeps.  The factor of two on top of it: the restatement steps
   the two tiles of the pocket together, the device visits them in turn, and a visit sees the other tile's labels only as they
   were when it loaded its halo.  A pixel on the border can therefore spend one visit relabelling against a label its neighbour
   has already left, i.e. at worst every useful visit of a tile is paired with one wasted on stale labels, and never more: the
   next visit loads the halo afresh.  That doubles the ceiling run's visits at worst; the run without the ceiling is bounded
   above by its chain budget either way.  The test requires the allowed ratio itself to be below one half.
   "Nothing active" is asserted three ways: no chain cut by the hop limit, at least one chain that ended with nothing to hand
   on, and the solve's round count equal to the restatement's (a launch that left active excess behind would need a further
   round to work it off)."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import maxflow_nets as mn

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
DINF = 1 << 29

# name -> [(family, variant, h, w)]: one entry is a single network, several are one batch
CASES = {
    "random_1x1": [("random", "dense", 1, 1)],
    "random_8x32": [("random", "dense", 8, 32)],
    "extremes_checker_8x32": [("extremes", "checker", 8, 32)],
    "random_9x33": [("random", "dense", 9, 33)],
    "corner_gates_9x33": [("corner_gates", "gates", 9, 33)],
    "random_40x70": [("random", "dense", 40, 70)],
    "extremes_one_sink_40x70": [("extremes", "one_sink", 40, 70)],
    "border_32x8_40x70": [("border_bottlenecks", "tiles_32x8", 40, 70)],
    "serpentine_96x128": [("serpentine", "mid_bottleneck", 96, 128)],
    "corner_gates_72x100": [("corner_gates", "gates", 72, 100)],
    "border_32x32_72x100": [("border_bottlenecks", "tiles_32x32", 72, 100)],
    "warm_72x100": [("warm", "resample", 72, 100)],
    "detour_8x32": [("detour", "", 8, 32)],
    "pocket_8x64": [("pocket", "", 8, 64)],
    "batch_of_five_72x100": [("random", "dense", 72, 100), ("corner_gates", "gates", 72, 100), ("degenerate", "all_sink", 72, 100),
                             ("border_bottlenecks", "tiles_32x8", 72, 100), ("serpentine", "mid_bottleneck", 72, 100)],
}
SCHEDULES = {
    "default": {},
    "all_async": {"GGC_MF_ASYNC_PUSH_ACTIVE": "100000000", "GGC_MF_RELAX_DENSE": "1", "GGC_MF_PARTIAL_ROUNDS": "0"},
    "all_dense": {"GGC_MF_ASYNC_PUSH_ACTIVE": "0"},
}
SLACKS = {"slack_0": {"GGC_MF_LABEL_SLACK": "0"}, "slack_4": {"GGC_MF_LABEL_SLACK": "4"}, "library_default": {},
          "ceiling_off": {"GGC_MF_LABEL_SLACK": "-1"}}
ASYNC_HOPS, ASYNC_SWEEPS = 127, 12

CHILD = r"""
import sys, time
sys.path[:0] = [r"{root}", r"{root}/src", r"{root}/tests"]
import numpy as np
from gcn_grabcut import _native
import maxflow_nets as mn
ctx = _native.get_context(0)
ref = np.load(r"{refs}")
names = {names!r}
for name in names:
    t0 = time.time()
    n = int(ref[name + "/n"])
    nets = [(ref[f"{{name}}/{{b}}/tw"], ref[f"{{name}}/{{b}}/nw"]) for b in range(n)]
    side, res = mn.solve(ctx, nets)
    for b, (tw, nw) in enumerate(nets):
        want = ref[f"{{name}}/{{b}}/cut"]
        for s in range(tw.shape[0]):
            assert np.array_equal(side[s, b], want[s]), (name, b, s, int((side[s, b] != want[s]).sum()))
        mn.certify(tw[-1], nw, side[-1, b], res[b], int(ref[f"{{name}}/{{b}}/flow"]), cold=tw.shape[0] == 1)
    print(f"case ok: {{name}} ({{time.time() - t0:.2f}} s)", flush=True)
"""


def _detour(h, w):
    """S = (3, 0) holds 100; T1 = (2, 0) above it behind a link of 5; a corridor of links of 1000 along row 3 to T2 = (3, w - 1)."""
    tw = np.zeros((1, h, w), np.int32)
    nw = np.zeros((4, h, w), np.int32)
    tw[0, 3, 0], tw[0, 2, 0], tw[0, 3, w - 1] = 100, -1000, -1000
    nw[2, 3, 0] = 5                                        # plane 2: the link of a pixel to the one above it
    nw[0, 3, 1:] = 1000                                    # plane 0: to the left
    return tw, nw


POCKET_X0, POCKET_X1 = 23, 41                              # the pocket's columns [x0, x1): across the tile border at x = 32


def _pocket(h, w):
    """Pocket: columns 23 .. 40 of every row, 5 per pixel, links of 100 inside.  One exit of 40 from (4, 40) to (4, 41); the
    open region is row 4, columns 41 .. 43, links of 1000, with a sink at (4, 43)."""
    tw = np.zeros((1, h, w), np.int32)
    nw = np.zeros((4, h, w), np.int32)
    tw[0, :, POCKET_X0:POCKET_X1] = 5
    ys, xs = np.mgrid[0:h, 0:w]
    for k, (dy, dx) in enumerate(mn.PLANE_OFF):
        inside = (xs >= POCKET_X0) & (xs < POCKET_X1) & (xs + dx >= POCKET_X0) & (xs + dx < POCKET_X1) & (ys + dy >= 0) & (ys + dy < h)
        nw[k][inside] = 100
    nw[0, 4, POCKET_X1] = 40
    nw[0, 4, POCKET_X1 + 1:POCKET_X1 + 3] = 1000
    tw[0, 4, POCKET_X1 + 2] = -100000
    return tw, nw


def _make(fam, var, h, w):
    return _detour(h, w) if fam == "detour" else _pocket(h, w) if fam == "pocket" else mn.make(fam, var, h, w, seed=47)


# ---------------------------------------------------------------------------------------------- the schedule, restated
def _relabel(rc, snk):
    """Exact distances to the sink in the residual graph, DINF where there is no way."""
    dist = np.where(snk > 0, 1, DINF).astype(np.int64)
    while True:
        new = dist
        for d, (dy, dx, _, _) in enumerate(mn.DIRS):
            new = np.minimum(new, np.where(rc[:, :, d] > 0, mn._shift(dist, dy, dx) + 1, DINF))
        if np.array_equal(new, dist):
            return dist
        dist = new


def _sweep(rc, ex, snk, dist, lim):
    """One synchronous step of every active pixel by the rule of push_tile_visit; False when none is active."""
    act = (ex > 0) & (dist < lim)
    if not act.any():
        return False
    hmin = np.where(snk > 0, 0, DINF).astype(np.int64)
    best = np.where(snk > 0, 8, -1)
    for d, (dy, dx, _, _) in enumerate(mn.DIRS):
        ok = (rc[:, :, d] > 0) & (mn._shift(dist, dy, dx) < hmin)
        hmin = np.where(ok, mn._shift(dist, dy, dx), hmin)
        best = np.where(ok, d, best)
    can = act & (best >= 0) & (dist > hmin)
    e0 = ex.copy()
    dl = np.where(can & (best == 8), np.minimum(e0, snk), 0)
    ex -= dl
    snk -= dl
    for d, (dy, dx, _, _) in enumerate(mn.DIRS):
        dl = np.where(can & (best == d), np.minimum(e0, rc[:, :, d]), 0)
        rc[:, :, d] -= dl
        ex -= dl
        got = mn._shift(dl, -dy, -dx)                      # what the pixel at the arc's head receives
        ex += got
        rc[:, :, d ^ 1] += got
    rel = act & ~can
    dist[rel] = np.where((best >= 0) & (hmin < DINF), hmin + 1, DINF)[rel]
    return True


def _simulate(tw, nw, slack, sweeps_of_round, max_rounds=32):
    """-> (rounds, [sweeps used by the push phase of each round], [parked pixels the relabel of each round found reachable])."""
    h, w = tw.shape
    rc = mn._arc_caps(nw)
    ex, snk = np.maximum(tw, 0).astype(np.int64), np.maximum(-tw, 0).astype(np.int64)
    sweeps, wrong = [], []
    parked = np.zeros((h, w), bool)
    for rnd in range(max_rounds):
        dist = _relabel(rc, snk)
        wrong.append(int((parked & (ex > 0) & (dist < DINF)).sum()))
        if not ((ex > 0) & (dist < DINF)).any():
            return rnd + 1, sweeps, wrong
        lmax = int(dist[dist < DINF].max())
        lim = h * w if slack < 0 else min(h * w, lmax + 1 + slack)
        n = 0
        while n < sweeps_of_round(rnd) and _sweep(rc, ex, snk, dist, lim):
            n += 1
        sweeps.append(n)
        parked = (ex > 0) & (dist >= lim) & (dist < DINF)
    raise AssertionError("the restated schedule did not end")


# ---------------------------------------------------------------------------------------------- device runs
@pytest.fixture(scope="module")
def refs(oracle, tmp_path_factory):
    """The networks, the oracle's cut of every step and the flow value of the last one, in one .npz for the children."""
    out = {}
    for name, nets in CASES.items():
        out[name + "/n"] = np.int64(len(nets))
        for b, (fam, var, h, w) in enumerate(nets):
            tw, nw = _make(fam, var, h, w)
            cuts = []
            for s in range(tw.shape[0]):
                flow, want = oracle.grid_maxflow(tw[s], nw)
                cuts.append(np.asarray(want, np.uint8))
            out[f"{name}/{b}/tw"], out[f"{name}/{b}/nw"] = tw, nw
            out[f"{name}/{b}/cut"], out[f"{name}/{b}/flow"] = np.stack(cuts), np.int64(flow)
    path = tmp_path_factory.mktemp("mf_ceiling") / "refs.npz"
    np.savez(path, **out)
    return path


def _run_child(refs, env_extra, names):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GGC_MF")}
    env.update(env_extra)
    code = CHILD.format(root=str(ROOT), refs=str(refs), names=list(names))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    print(r.stdout)
    missing = [n for n in names if f"case ok: {n} " not in r.stdout]
    assert r.returncode == 0 and not missing, f"rc {r.returncode}, not passed: {missing}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return r


def _rounds(stderr):
    return len(re.findall(r"\[ggc maxflow\] round \d+:", stderr))


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("slack", list(SLACKS))
def test_ceiling_matches_oracle_and_certifies(refs, slack, schedule):
    _run_child(refs, dict(SCHEDULES[schedule], **SLACKS[slack]), list(CASES))


def test_detour_is_parked_and_released(refs):
    tw, nw = _detour(8, 32)
    sim = {s: _simulate(tw[0], nw, s, lambda rnd: 1 << 20) for s in (0, -1)}
    print("restated schedule (rounds, sweeps per round, parked-but-reachable per relabel): ceiling", sim[0], "off", sim[-1])
    assert sim[0][0] == 3 and sim[-1][0] == 2 and max(sim[0][2]) > 0 and max(sim[-1][2]) == 0
    n_sweeps = 4 * max(sim[0][1] + sim[-1][1])
    env = dict(SCHEDULES["all_dense"], GGC_MF_DENSE_LAUNCHES0="1", GGC_MF_DENSE_LAUNCHES="1", GGC_MF_DENSE_SWEEPS=str(n_sweeps),
               GGC_MF_PARTIAL_ROUNDS="0", GGC_MF_TRACE="1")
    got = {}
    for s in (0, -1):
        r = _run_child(refs, dict(env, GGC_MF_LABEL_SLACK=str(s)), ["detour_8x32"])
        wrong = [int(x) for x in re.findall(r"\[ceiling\] .*of them finite after the relabel (\d+)", r.stderr)]
        got[s] = (_rounds(r.stderr), wrong)
    print("device (rounds, parked-but-reachable per relabel): ceiling", got[0], "off", got[-1], "sweeps per visit", n_sweeps)
    assert sum(got[0][1]) > 0, "no parked excess went through a relabel: the network did not exercise the ceiling"
    assert sum(got[-1][1]) == 0, "excess counted as parked with the ceiling off"
    assert 1 <= got[-1][0] <= sim[-1][0], f"{got[-1][0]} rounds with the ceiling off"
    assert got[-1][0] < got[0][0] <= sim[0][0], f"{got[0][0]} rounds with the ceiling against {got[-1][0]} without; restated: {sim[0][0]}"


def test_sealed_pocket_retires_below_the_ceiling(refs):
    tw, nw = _pocket(8, 64)
    budget = ASYNC_HOPS * ASYNC_SWEEPS
    sim = {s: _simulate(tw[0], nw, s, lambda rnd: 1 if rnd == 0 else budget) for s in (0, -1)}
    s_lim, s_off = sim[0][1][1], sim[-1][1][1]
    allowed = 2.0 * s_lim / s_off
    print("restated schedule: sweeps of round 1 with the ceiling", s_lim, "without", s_off, "of a budget of", budget, "allowed ratio of visits", allowed)
    assert s_lim < budget and allowed < 0.5
    env = dict(SCHEDULES["all_async"], GGC_MF_ASYNC_HOPS=str(ASYNC_HOPS), GGC_MF_ASYNC_SWEEPS=str(ASYNC_SWEEPS), GGC_MF_DENSE_LAUNCHES0="1",
               GGC_MF_DENSE_SWEEPS="1", GGC_MF_TRACE="1")
    got = {}
    for s in (0, -1):
        r = _run_child(refs, dict(env, GGC_MF_LABEL_SLACK=str(s)), ["pocket_8x64"])
        lines = re.findall(r"\[async push\] \d+ waves alive [\d.]+ us on average; (\d+) visits .*chains cut by the hop limit (\d+), ended with nothing to hand on (\d+)", r.stderr)
        assert lines, f"no asynchronous push launch ran\n{r.stderr[-3000:]}"
        got[s] = (sum(int(v) for v, _, _ in lines), sum(int(c) for _, c, _ in lines), _rounds(r.stderr), sum(int(i) for _, _, i in lines))
    print("device (asynchronous visits, chains cut by the hop limit, rounds, chains ended idle): ceiling", got[0], "off", got[-1])
    assert got[0][1] == 0, f"{got[0][1]} chains ran into the hop limit under the ceiling"
    assert got[0][3] > 0, "no chain of the ceiling run ended with nothing to hand on"
    assert got[0][2] == sim[0][0], f"{got[0][2]} rounds under the ceiling, the restated schedule needs {sim[0][0]}"
    assert got[0][0] <= allowed * got[-1][0], f"{got[0][0]} visits with the ceiling, {got[-1][0]} without, allowed ratio {allowed:.3f}"
