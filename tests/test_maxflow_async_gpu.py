"""The asynchronous max-flow phases at the shapes where their tile hops can go wrong.

The push visit carries a lane's next pixel in a register and spills to an LDS mask only what it cannot carry; the queue of
either asynchronous launch starts from the work list of the kernel before it, with ring, control words and tile state words
prepared by k_mf_rinit / k_mf_active (csrc/ggc_maxflow_async.hip).  The settings below push all sparse and most dense work
through those kernels:

  all_async           GGC_MF_ASYNC_PUSH_ACTIVE=100000000 GGC_MF_RELAX_DENSE=1 GGC_MF_PARTIAL_ROUNDS=0
  all_async_one_hop   the same with GGC_MF_ASYNC_HOPS=1: nothing is followed or queued onwards, a round ends after one hop
  all_async_one_sweep the same with GGC_MF_ASYNC_SWEEPS=1: every pixel spills or is carried exactly once per visit

The library reads its GGC_MF_* switches once per process, so each setting runs in one child interpreter (one at a time, with
a time limit).  Every network goes through ggc_grid_maxflow (tests/maxflow_nets.py): every step's cut must equal the CPU
oracle's, and the final state must pass the max-flow/min-cut certificate.  The oracle's cuts are computed once, in this
process, and handed to the children in a file.

Shapes: 1x1; 8x32 (exactly one push tile, no neighbour, a list count of 0 or 1); 9x33 (four push tiles, three of them
one-pixel slivers, relabel and push tiles overhanging the image); 40x70 (ragged both ways); the 96x128 serpentine (long
chains, followed hops, the hop cap); corner gates and both border-bottleneck variants at 72x100 (hand-overs across corners,
border arcs re-opened under a held tile); the warm family at 72x100; and one batch of five networks of different kinds at
72x100 in which one image (all_sink) has nothing active from the start: a closed image whose state words must never be read
as queued, and a list count smaller than the grid.  The default schedule runs that batch twice in one process and must get
identical cuts: state left behind in the ring or in the state words by the launch before would show there.

The cut cannot tell whether a visit works its pixels off or leaves them to later visits: excess that a visit forgets is
found again by the next visit's fill or the next round's active scan.  test_remainder_is_worked_within_the_visit therefore
counts ROUNDS on a fan: one source pixel holding 8 c of excess in the middle of an 8x32 tile, eight neighbours with a sink
link of c each, links of capacity c.  Every push of the source saturates its arc and leaves a remainder while its lane goes
on with the receiver.  The dense first round is cut down to one launch of one sweep (one push), chains to one hop; then one
visit of 12 sweeps drains the fan (seven pushes of the source, each receiver's push into its sink link a sweep later: 8
sweeps), so the solve prints three rounds: the dense one, the asynchronous one, and the one that finds nothing active.  A
visit that drops the remainder gets one push of the source per round: nine rounds.  Bound: 4."""
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

# name -> [(family, variant, h, w)]: one entry is a single network, several are one batch
CASES = {
    "random_1x1": [("random", "dense", 1, 1)],
    "random_8x32": [("random", "dense", 8, 32)],
    "all_sink_8x32": [("degenerate", "all_sink", 8, 32)],
    "random_9x33": [("random", "dense", 9, 33)],
    "corner_gates_9x33": [("corner_gates", "gates", 9, 33)],
    "random_40x70": [("random", "dense", 40, 70)],
    "border_32x8_40x70": [("border_bottlenecks", "tiles_32x8", 40, 70)],
    "serpentine_96x128": [("serpentine", "mid_bottleneck", 96, 128)],
    "corner_gates_72x100": [("corner_gates", "gates", 72, 100)],
    "border_32x8_72x100": [("border_bottlenecks", "tiles_32x8", 72, 100)],
    "border_32x32_72x100": [("border_bottlenecks", "tiles_32x32", 72, 100)],
    "warm_72x100": [("warm", "resample", 72, 100)],
    "fan_8x32": [("fan", "", 8, 32)],
    "batch_of_five_72x100": [("random", "dense", 72, 100), ("corner_gates", "gates", 72, 100), ("degenerate", "all_sink", 72, 100),
                             ("border_bottlenecks", "tiles_32x8", 72, 100), ("serpentine", "mid_bottleneck", 72, 100)],
}
ALL_ASYNC = {"GGC_MF_ASYNC_PUSH_ACTIVE": "100000000", "GGC_MF_RELAX_DENSE": "1", "GGC_MF_PARTIAL_ROUNDS": "0"}
SETTINGS = {
    "all_async": dict(ALL_ASYNC),
    "all_async_one_hop": dict(ALL_ASYNC, GGC_MF_ASYNC_HOPS="1"),
    "all_async_one_sweep": dict(ALL_ASYNC, GGC_MF_ASYNC_SWEEPS="1"),
}

CHILD = r"""
import sys, time
sys.path[:0] = [r"{root}", r"{root}/src", r"{root}/tests"]
import numpy as np
from gcn_grabcut import _native
import maxflow_nets as mn
ctx = _native.get_context(0)
ref = np.load(r"{refs}")
names = {names!r}
repeat = {repeat}
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
    for k in range(repeat):
        again, _ = mn.solve(ctx, nets, residual=False)
        assert np.array_equal(again, side), (name, "call", k + 2, int((again != side).sum()))
    print(f"case ok: {{name}} ({{time.time() - t0:.2f}} s)", flush=True)
"""


def _fan(h, w, c=100):
    """One source of 8 c at (h / 2, w / 2), its eight neighbours with a sink link of c, the eight links of capacity c."""
    cy, cx = h // 2, w // 2
    tw = np.zeros((1, h, w), np.int32)
    nw = np.zeros((4, h, w), np.int32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                tw[0, cy + dy, cx + dx] = -c
    tw[0, cy, cx] = 8 * c
    for k, (dy, dx) in enumerate(mn.PLANE_OFF):            # plane k of p links p and p + (dy, dx)
        nw[k, cy, cx] = c
        nw[k, cy - dy, cx - dx] = c
    return tw, nw


def _make(fam, var, h, w):
    return _fan(h, w) if fam == "fan" else mn.make(fam, var, h, w, seed=31)


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
    path = tmp_path_factory.mktemp("mf_async") / "refs.npz"
    np.savez(path, **out)
    return path


def _run_child(refs, env_extra, names, repeat=0):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GGC_MF")}
    env.update(env_extra)
    code = CHILD.format(root=str(ROOT), refs=str(refs), names=list(names), repeat=repeat)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    print(r.stdout)
    missing = [n for n in names if f"case ok: {n} " not in r.stdout]
    assert r.returncode == 0 and not missing, f"rc {r.returncode}, not passed: {missing}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return r


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_asynchronous_schedule_matches_oracle_and_certifies(refs, setting):
    _run_child(refs, SETTINGS[setting], list(CASES))


def test_default_schedule_twice_in_one_process_gives_identical_cuts(refs):
    _run_child(refs, {}, ["batch_of_five_72x100"], repeat=1)


def test_remainder_is_worked_within_the_visit(refs):
    env = dict(SETTINGS["all_async_one_hop"], GGC_MF_DENSE_LAUNCHES0="1", GGC_MF_DENSE_SWEEPS="1", GGC_MF_TRACE="1")
    r = _run_child(refs, env, ["fan_8x32"])
    rounds = len(re.findall(r"\[ggc maxflow\] round \d+:", r.stderr))
    print("rounds", rounds)
    assert 1 <= rounds <= 4, f"{rounds} rounds for the fan\n{r.stderr[-3000:]}"
