"""The device max-flow on networks built to break it (tests/maxflow_nets.py), through ggc_grid_maxflow: the production solver
of ggc_grabcut, fed a caller's t-links and n-links.

For every network and step the device's source side must equal the CPU oracle's canonical cut bit for bit, and the final
residual state must carry a max-flow/min-cut certificate in exact integer arithmetic (maxflow_nets.certify): non-negative
arcs, intact link pairs, conserved flow, no excess that can still reach the sink, the cut read off that state, and a cut
capacity equal to the oracle's flow value.

Serpentine sizes, from one GGC_MF_TRACE=1 run of the default schedule on an MI355X (cold solve, B = 1):
  96 x 128  (corridor of 6 191 pixels):   28 rounds, the first 3 partial
  240 x 320 (corridor of 38 519 pixels): 155 rounds, the first 3 partial
far below the driver's cap of 4096 rounds; the whole file runs in well under a minute."""
import numpy as np
import pytest

import maxflow_nets as mn

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 257), (257, 1), (2, 33), (7, 9), (8, 32), (32, 8), (33, 65), (31, 97), (200, 272), (480, 640)]
SERPENTINES = [(96, 128), (240, 320)]
FAMILIES = [f for f in mn.VARIANTS if f != "serpentine"]


def _check(oracle, nets, side, res, label):
    """side (S, B, H, W) and res (B, H, W, 10) of a batch against the oracle, step by step, and the final certificate."""
    for b, (tw, nw) in enumerate(nets):
        n_steps = tw.shape[0]
        for s in range(n_steps):
            flow, want = oracle.grid_maxflow(tw[s], nw)
            got = side[s, b]
            assert np.array_equal(got, want), f"{label} image {b} step {s}: {int((got != want).sum())} pixels differ"
        mn.certify(tw[-1], nw, side[-1, b], res[b], flow, cold=n_steps == 1)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("h,w", SHAPES)
def test_family_matches_oracle_and_certifies(gpu_ctx, oracle, family, h, w):
    nets = [mn.make(family, v, h, w, seed=11) for v in mn.VARIANTS[family]]
    side, res = mn.solve(gpu_ctx, nets)
    _check(oracle, nets, side, res, f"{family} {h}x{w}")


@pytest.mark.parametrize("h,w", SERPENTINES)
def test_serpentine_matches_oracle_and_certifies(gpu_ctx, oracle, h, w):
    nets = [mn.make("serpentine", "mid_bottleneck", h, w)]
    side, res = mn.solve(gpu_ctx, nets)
    _check(oracle, nets, side, res, f"serpentine {h}x{w}")
    assert res[0, :, :, 8].sum() > 0                       # excess stays trapped behind the bottleneck


def test_batch_of_70_equals_single_solves(gpu_ctx, oracle):
    """More than 64 open images (the driver's grids scale by 64), one long serpentine that keeps the open list at a single
    image for most rounds, and random and degenerate networks that close early."""
    h, w = SERPENTINES[0]
    nets = [mn.make("serpentine", "mid_bottleneck", h, w)]
    kinds = [("random", v) for v in mn.VARIANTS["random"]] + [("degenerate", v) for v in mn.VARIANTS["degenerate"]]
    for i in range(69):
        f, v = kinds[i % len(kinds)]
        nets.append(mn.make(f, v, h, w, seed=100 + i))
    side, res = mn.solve(gpu_ctx, nets)
    _check(oracle, nets, side, res, "batch of 70")
    for b in (0, 1, 2, 3, 35, 69):
        one, _ = mn.solve(gpu_ctx, [nets[b]])
        assert np.array_equal(one[:, 0], side[:, b]), f"image {b} of the batch differs from its own solve"


def test_two_calls_give_identical_cuts(gpu_ctx, oracle):
    """The cut is canonical, the final preflow is not: the lock-free pushes race (LDS atomics of concurrent waves, global
    deltas of neighbouring tiles, the ticket order of the asynchronous launches), so two calls may leave different excess
    pockets — on an MI355X they do.  Both must be maximum preflows of the same network with the same cut."""
    tw, nw = mn.make("warm", "resample", 200, 272, seed=5)
    nets = [mn.make("border_bottlenecks", "tiles_32x8", 200, 272, seed=5), mn.make("corner_gates", "gates", 200, 272, seed=5),
            (tw[:1], nw)]
    side1, res1 = mn.solve(gpu_ctx, nets)
    side2, res2 = mn.solve(gpu_ctx, nets)
    assert np.array_equal(side1, side2)
    _check(oracle, nets, side1, res1, "first call")
    _check(oracle, nets, side2, res2, "second call")


@pytest.mark.parametrize("family", ["random", "corner_gates", "border_bottlenecks", "extremes", "warm"])
@pytest.mark.parametrize("h,w", [(33, 65), (200, 272)])
def test_seed_sweep(gpu_ctx, oracle, family, h, w):
    """Twelve draws of every variant in one batch."""
    nets = [mn.make(family, v, h, w, seed=1000 + s) for s in range(12) for v in mn.VARIANTS[family]]
    side, res = mn.solve(gpu_ctx, nets)
    _check(oracle, nets, side, res, f"{family} {h}x{w} sweep")


def _call(gpu_ctx, tw, nw, B=None, H=None, W=None, S=None):
    import torch
    from gcn_grabcut import _native
    s, b, h, w = tw.shape
    dtw, dnw = torch.as_tensor(tw).cuda(), torch.as_tensor(nw).cuda()
    side = torch.full((s, b, h, w), 255, dtype=torch.uint8, device="cuda")
    with pytest.raises(_native.GGCError) as e:
        gpu_ctx.call("ggc_grid_maxflow", _native.current_stream(0), b if B is None else B, h if H is None else H,
                     w if W is None else W, s if S is None else S, dtw.data_ptr(), dnw.data_ptr(), side.data_ptr(), None)
    assert e.value.code == -1, e.value                    # GGC_E_INVALID_ARG
    assert (side == 255).all(), "a rejected call wrote its output"


def test_rejects_out_of_range_inputs(gpu_ctx):
    tw0, nw0 = mn.to_device([mn.make("random", "dense", 33, 40, seed=1), mn.make("random", "dense", 33, 40, seed=2)])
    for y, x, v in [(5, 7, mn.TW_MAX + 1), (32, 39, -mn.TW_MAX - 1), (0, 0, -(1 << 31))]:
        tw = tw0.copy(); tw[0, 1, y, x] = v
        _call(gpu_ctx, tw, nw0)
    for k, y, x, v in [(0, 3, 4, -1), (3, 32, 0, mn.NW_MAX + 1), (2, 1, 39, -(1 << 31))]:
        nw = nw0.copy(); nw[k, 1, y, x] = v
        _call(gpu_ctx, tw0, nw)
    _call(gpu_ctx, tw0, nw0, B=0)
    _call(gpu_ctx, tw0, nw0, H=0)
    _call(gpu_ctx, tw0, nw0, W=0)
    _call(gpu_ctx, tw0, nw0, S=0)
