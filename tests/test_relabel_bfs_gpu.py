"""The dense relabel launches with the BFS tile visit (mf_relax_visit_bfs, ggc_mf_sweep.h), through the production solver.

ggc_grid_maxflow on the networks of tests/maxflow_nets.py: the device's source side must be the CPU oracle's canonical cut
at every step, and the final residual state must carry the exact max-flow/min-cut certificate (maxflow_nets.certify).
The shapes are the smallest that reach every path of the visit: 1x1 (one pixel, everything else outside the image), 31x33
and 33x65 (tiles cut by the right and bottom image border, halos that cross tile borders), 96x128 (3 x 4 whole tiles, fronts
that enter a tile from a neighbour several times).  The serpentine's corridor is 1 024 pixels long inside a tile — far above
the level cap, so its visits must hand over to the sweeps — and the corner-gate walls let a front into a tile only through
the diagonal arcs of its corner pixels.  A batch of 3 puts tiles of different images into one launch.

One GrabCut run (64 x 96, batch of 3) is certified iteration by iteration against the float64 GrabCut of grabcut_ref.py."""
import numpy as np
import pytest

import grabcut_ref as gr
import maxflow_nets as mn
from test_grabcut_gpu import _grabcut, _trimaps

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (31, 33), (33, 65), (96, 128)]
FAMILIES = [f for f in mn.VARIANTS if f != "serpentine"]


def _check(oracle, nets, side, res, label):
    for b, (tw, nw) in enumerate(nets):
        n_steps = tw.shape[0]
        for s in range(n_steps):
            flow, want = oracle.grid_maxflow(tw[s], nw)
            got = side[s, b]
            assert np.array_equal(got, want), f"{label} image {b} step {s}: {int((got != want).sum())} pixels differ"
        mn.certify(tw[-1], nw, side[-1, b], res[b], flow, cold=n_steps == 1)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("h,w", SHAPES)
def test_family_cut_and_certificate(gpu_ctx, oracle, family, h, w):
    nets = [mn.make(family, v, h, w, seed=31) for v in mn.VARIANTS[family]]
    side, res = mn.solve(gpu_ctx, nets)
    _check(oracle, nets, side, res, f"{family} {h}x{w}")


def test_serpentine_takes_the_fallback(gpu_ctx, oracle):
    nets = [mn.make("serpentine", "mid_bottleneck", 96, 128)]
    side, res = mn.solve(gpu_ctx, nets)
    _check(oracle, nets, side, res, "serpentine 96x128")
    assert res[0, :, :, 8].sum() > 0                       # excess stays trapped behind the bottleneck


@pytest.mark.parametrize("h,w", [(33, 65), (96, 128)])
def test_batch_of_3(gpu_ctx, oracle, h, w):
    """A corridor tile (fallback), corner-diagonal walls and a random network side by side in the same launches."""
    nets = [mn.make("serpentine", "mid_bottleneck", h, w), mn.make("corner_gates", "gates", h, w, seed=32),
            mn.make("random", "dense", h, w, seed=33)]
    side, res = mn.solve(gpu_ctx, nets)
    _check(oracle, nets, side, res, f"batch of 3 {h}x{w}")
    for b in range(3):
        one, _ = mn.solve(gpu_ctx, [nets[b]])
        assert np.array_equal(one[:, 0], side[:, b]), f"image {b} of the batch differs from its own solve"


def test_grabcut_batch_certified(oracle, gpu_ctx):
    from gcn_grabcut.synthetic import synthetic_image
    h, w, b, seed = 64, 96, 3, 11
    pairs = [synthetic_image(h, w, 7600 + i, return_mask=True) for i in range(b)]
    imgs = np.stack([p[0] for p in pairs])
    tris = _trimaps(imgs, [p[1] for p in pairs])
    states = []
    for k in range(3):                                      # set-up, the cold solve, one warm-started solve
        _, m, bg, fg = _grabcut(gpu_ctx, imgs, tris, n_iter=k, mode=0, seed=seed)
        states.append((m, bg, fg))
    for i in range(b):
        assert np.array_equal(states[0][0][i], gr.init_trimap(tris[i])[0])
        for k in (1, 2):
            gr.certify_step(oracle, imgs[i], *(s[i] for s in states[k - 1]), *(s[i] for s in states[k]), what=f"[{i}] it{k}")
