"""GPU parity for the two fused edge-aware trimap kernels (radius 1..8): bit-exact against the CPU oracle.

The inputs are hand-made (no SLIC): a grid of 5 x 7-pixel regions, probabilities down to 1e-15 with exact zeros (so the
float64 summation order matters), and an image with a constant patch (zero variance) and a black quadrant (zero guide).
The shapes run from images smaller than the filter radius (repeated reflection) over exactly one 32 x 32 tile to one
pixel past a tile in each direction.
"""
import numpy as np
import pytest
import torch

import gpu_helpers as gh

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 3), (3, 5), (9, 9), (31, 33), (32, 64), (33, 65), (64, 128), (97, 130)]
RADII = [1, 2, 5, 8]
ALL_LABELS = [(64, 128), (97, 130)]          # here the oracle's trimap must hold all four labels at every radius
THR, EPS = 0.55, 1e-3


def _inputs(h, w, r, extra=0):
    rng = np.random.default_rng(h * 1000 + w + r + extra)
    yy, xx = np.mgrid[0:h, 0:w]
    seg = ((yy // 5) * -(-w // 7) + xx // 7).astype(np.int32)
    n = int(seg.max()) + 1
    logits = (6 * rng.standard_normal((n, 3))).astype(np.float32)
    e = np.exp(logits - logits.max(1, keepdims=True))
    probs = (e / e.sum(1, keepdims=True)).astype(np.float32)
    probs[::7, 0] = 0.0
    bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    bgr[:h // 3, :w // 2] = 90               # zero variance
    bgr[h // 2:, w // 2:] = 0                # zero guide
    return probs, seg, bgr


def _refine(ctx, probs, node_ptr, seg, bgr, radius):
    b, h, w = seg.shape
    args = [torch.as_tensor(np.ascontiguousarray(a)).cuda() for a in (probs, node_ptr, seg, bgr)]
    tri = torch.full((b, h, w), 255, dtype=torch.uint8, device="cuda")
    ctx.call("ggc_refine_trimap", gh.stream(), b, h, w, args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(),
             args[3].data_ptr(), THR, THR, radius, EPS, 1, tri.data_ptr())
    return tri.cpu().numpy()


def _check_one(oracle, ctx, h, w, radius):
    probs, seg, bgr = _inputs(h, w, radius)
    want = oracle.refine_trimap(probs, seg, bgr, THR, THR, radius, EPS, True)
    if (h, w) in ALL_LABELS and radius <= 8:
        assert sorted(np.unique(want)) == [0, 1, 2, 3], np.bincount(want.ravel(), minlength=4)
    node_ptr = np.array([0, probs.shape[0]], np.int32)
    got = _refine(ctx, probs, node_ptr, seg[None], bgr[None], radius)[0]
    assert np.array_equal(got, want), (h, w, radius, int((got != want).sum()))


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("h,w", SHAPES)
def test_fused_trimap_bit_exact(oracle, gpu_ctx, h, w, radius):
    _check_one(oracle, gpu_ctx, h, w, radius)


def test_radius_above_eight_takes_the_plane_by_plane_route(oracle, gpu_ctx):
    _check_one(oracle, gpu_ctx, 33, 65, 9)


def test_fused_trimap_batch_of_three(oracle, gpu_ctx):
    """Three different images in one call: a block that read another image's planes or probabilities would show."""
    h, w, radius = 33, 65, 8
    parts = [_inputs(h, w, radius, extra) for extra in (0, 1, 2)]
    node_ptr = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in parts])]).astype(np.int32)
    got = _refine(gpu_ctx, np.concatenate([p[0] for p in parts]), node_ptr, np.stack([p[1] for p in parts]),
                  np.stack([p[2] for p in parts]), radius)
    wants = [oracle.refine_trimap(p[0], p[1], p[2], THR, THR, radius, EPS, True) for p in parts]
    assert not np.array_equal(wants[0], wants[1]) and not np.array_equal(wants[1], wants[2])
    for i in range(3):
        assert np.array_equal(got[i], wants[i]), (i, int((got[i] != wants[i]).sum()))
