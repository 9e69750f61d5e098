"""The dense push launches of the max-flow (k_mf_pr_wave: a wave per 32x8 tile, the carried-pixel visit of
csrc/ggc_mf_push.h with plain loads and stores) at the shapes where that visit can go wrong.

By default only the first rounds of a solve are dense; the settings below send every push round through the kernel:

  all_dense              GGC_MF_ASYNC_PUSH_ACTIVE=0
  all_dense_long_visits  the same with GGC_MF_DENSE_SWEEPS=64: excess crosses whole tiles within a visit and piles up
  all_dense_one_sweep    the same with GGC_MF_DENSE_SWEEPS=1: every pixel is dealt, carried or spilled exactly once per visit
                         (small networks only: at one push per launch a long corridor would approach the round cap of 4096;
                         a CPU simulation of the schedule — exact relabel, then 8 or 12 launches of one synchronous push
                         step per active pixel — needs 1 / 7 / 3 / 7 / 4 / 3 / 3 rounds for the seven networks of
                         ONE_SWEEP_CASES; the visit works at most 64 of a tile's 256 pixels per sweep, so four times that
                         at worst)

The library reads its GGC_MF_* switches once per process, so each setting runs in one child interpreter (one at a time, with
a time limit).  Every network goes through ggc_grid_maxflow (tests/maxflow_nets.py): every step's cut must equal the CPU
oracle's, and the final state must pass the max-flow/min-cut certificate.  The oracle's cuts are computed once, in this
process, and handed to the children in a file.

Shapes: 1x1; 8x32 (exactly one tile: three of the block's four waves idle); 9x33 (four tiles, three of them slivers: clamped
loads, lanes outside the image); 40x70; the 96x128 serpentine; corner gates at 9x33 and 72x100; both border-bottleneck
variants and the warm family at 72x100; the batch of five at 72x100 with its closed all_sink image; and two networks built
here in which every pixel holds excess and the only sink links are in one column: full_tile_8x32 (248 active pixels in one
tile: the mask stays non-empty for many sweeps, every sweep deals, bits beyond the first 64 stay behind) and
full_tiles_16x64 (the same over four tiles with the sink column in one of them: spills together with pushes across tile
edges and corners).  The default schedule runs the batch of five twice in one process and must get identical cuts.

The cut cannot see a remainder that a visit forgets (the next visit's fill or the next round's scan finds it again), so
test_one_visit_drains_the_fan counts ROUNDS: the fan of test_maxflow_async_gpu.py at 8x32, every round dense and cut down to
one launch of 12 sweeps.  The source pushes once per sweep (eight pushes, the last receiver's push into its sink link a sweep
later), so one visit drains the fan and the trace shows two rounds; a visit that drops the remainders gets one push of the
source per round: nine rounds.  Bound: 3.  The count is of rounds that can close the image, so the test also sets
GGC_MF_PARTIAL_ROUNDS=0: the default's first three rounds relabel partially and never close an image, which puts a floor of
four rounds under every solve, whatever its visits do (measured: 4 with this kernel and with k_mf_pr_list, the fan drained
in round 0 both times).

The fan never fills the spill mask.  A tile with more than 64 active pixels does: its sweeps must deal the lanes new pixels from the
mask, or the 64 lanes keep the pixels of the visit's first deal and everything else waits for the next visit's fill.
test_full_tiles_are_dealt_again counts the rounds of full_tile_8x32 and full_tiles_16x64 under the same settings with 64 sweeps per
visit.  A CPU simulation of that schedule (exact relabel, one visit per tile and round, per sweep one synchronous push step for the
first 64 active pixels of the tile in row-major order) needs 3 rounds for either network, and 12 / 11 when a visit keeps the 64 pixels
of its first sweep; with every active pixel stepping per sweep, as in k_mf_pr_list, 2.  The device's pushes race and its lanes carry
pixels in another order than the simulation deals them, so the bound is twice the simulated count: 6.  (Measured once: 3 / 3 with
k_mf_pr_wave, 2 / 3 with k_mf_pr_list, 10 / 10 with a library whose visit skips the deal.)"""
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
    "full_tile_8x32": [("full", "", 8, 32)],
    "random_9x33": [("random", "dense", 9, 33)],
    "corner_gates_9x33": [("corner_gates", "gates", 9, 33)],
    "full_tiles_16x64": [("full", "", 16, 64)],
    "fan_8x32": [("fan", "", 8, 32)],
    "random_40x70": [("random", "dense", 40, 70)],
    "serpentine_96x128": [("serpentine", "mid_bottleneck", 96, 128)],
    "corner_gates_72x100": [("corner_gates", "gates", 72, 100)],
    "border_32x8_72x100": [("border_bottlenecks", "tiles_32x8", 72, 100)],
    "border_32x32_72x100": [("border_bottlenecks", "tiles_32x32", 72, 100)],
    "warm_72x100": [("warm", "resample", 72, 100)],
    "batch_of_five_72x100": [("random", "dense", 72, 100), ("corner_gates", "gates", 72, 100), ("degenerate", "all_sink", 72, 100),
                             ("border_bottlenecks", "tiles_32x8", 72, 100), ("serpentine", "mid_bottleneck", 72, 100)],
}
ONE_SWEEP_CASES = ["random_1x1", "random_8x32", "full_tile_8x32", "random_9x33", "corner_gates_9x33", "full_tiles_16x64", "fan_8x32"]
ALL_DENSE = {"GGC_MF_ASYNC_PUSH_ACTIVE": "0"}
SETTINGS = {
    "all_dense": (dict(ALL_DENSE), list(CASES)),
    "all_dense_long_visits": (dict(ALL_DENSE, GGC_MF_DENSE_SWEEPS="64"), list(CASES)),
    "all_dense_one_sweep": (dict(ALL_DENSE, GGC_MF_DENSE_SWEEPS="1"), ONE_SWEEP_CASES),
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


def _full(h, w):
    """Every pixel holds excess (3 .. 9) but for rows 0 .. 7 of one column, which have the only sink links; links of 1 .. 12.
    8x32: column 20 of the only tile.  16x64: column 40, in the upper right of four tiles."""
    rng = np.random.default_rng(1000 * h + w)
    tw = rng.integers(3, 10, size=(1, h, w)).astype(np.int32)
    tw[0, :8, 20 if w <= 32 else 40] = -rng.integers(100, 200, size=8)
    nw = np.where(mn.in_image(h, w), rng.integers(1, 13, size=(4, h, w)), 0).astype(np.int32)
    return tw, nw


def _make(fam, var, h, w):
    return _fan(h, w) if fam == "fan" else _full(h, w) if fam == "full" else mn.make(fam, var, h, w, seed=31)


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
    path = tmp_path_factory.mktemp("mf_dense_wave") / "refs.npz"
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
def test_dense_schedule_matches_oracle_and_certifies(refs, setting):
    env, names = SETTINGS[setting]
    _run_child(refs, env, names)


def test_default_schedule_twice_in_one_process_gives_identical_cuts(refs):
    _run_child(refs, {}, ["batch_of_five_72x100"], repeat=1)


def test_one_visit_drains_the_fan(refs):
    env = dict(ALL_DENSE, GGC_MF_DENSE_LAUNCHES0="1", GGC_MF_DENSE_LAUNCHES="1", GGC_MF_DENSE_SWEEPS="12", GGC_MF_TRACE="1",
               GGC_MF_PARTIAL_ROUNDS="0")
    r = _run_child(refs, env, ["fan_8x32"])
    rounds = len(re.findall(r"\[ggc maxflow\] round \d+:", r.stderr))
    print("rounds", rounds)
    assert 1 <= rounds <= 3, f"{rounds} rounds for the fan\n{r.stderr[-3000:]}"


@pytest.mark.parametrize("name", ["full_tile_8x32", "full_tiles_16x64"])
def test_full_tiles_are_dealt_again(refs, name):
    env = dict(ALL_DENSE, GGC_MF_DENSE_LAUNCHES0="1", GGC_MF_DENSE_LAUNCHES="1", GGC_MF_DENSE_SWEEPS="64", GGC_MF_TRACE="1",
               GGC_MF_PARTIAL_ROUNDS="0")
    r = _run_child(refs, env, [name])
    rounds = len(re.findall(r"\[ggc maxflow\] round \d+:", r.stderr))
    print("rounds", name, rounds)
    assert 1 <= rounds <= 6, f"{rounds} rounds for {name}\n{r.stderr[-3000:]}"
