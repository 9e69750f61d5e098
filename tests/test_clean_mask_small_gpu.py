"""ggc_clean_mask against the CPU oracle on small masks built around the 8-neighbour joins of its labelling (csrc/ggc_ccl.h):
runs across the 64-pixel wave boundary in batches whose images do not start on one (with an empty and a full image, for
the per-image foreground flags of a wave that straddles two images), one-pixel-wide images, one-pixel staircases in both
diagonal directions across columns 62-66 (8-connected, not 4-connected), a comb whose teeth see a set pixel to the left,
above and above right, and two components of equal area, of which the first in raster order is the largest."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RULES = ((0.002, 0), (0.01, 0), (0.9, 0), (0.0, 1), (0.0, 0), (0.002, 1))     # those of test_grabcut_gpu.py


def _clean(gpu_ctx, masks, ratio, keep):
    from gcn_grabcut import _native
    masks = np.ascontiguousarray(masks, dtype=np.uint8)
    b, h, w = masks.shape
    d = torch.as_tensor(masks).cuda()
    out = torch.empty_like(d)
    gpu_ctx.call("ggc_clean_mask", _native.current_stream(0), b, h, w, d.data_ptr(), float(ratio), int(keep), out.data_ptr())
    return out.cpu().numpy()


def _check(oracle, gpu_ctx, masks):
    masks = np.ascontiguousarray(masks, dtype=np.uint8)
    for ratio, keep in RULES:
        got = _clean(gpu_ctx, masks, ratio, keep)
        for i in range(masks.shape[0]):
            want = oracle.clean_mask(masks[i], ratio, bool(keep))
            assert np.array_equal(got[i], want), (masks.shape, ratio, keep, i, int((got[i] != want).sum()))


def _random(b, h, w, seed):
    return (np.random.default_rng(seed).random((b, h, w)) < 0.3).astype(np.uint8)


@pytest.mark.parametrize("w", [63, 64, 65, 129])
def test_random_masks_across_the_wave_boundary(oracle, gpu_ctx, w):
    masks = _random(4, 21, w, seed=w)
    masks[1] = 0                                                    # no foreground: returned as it is
    masks[2] = 1                                                    # one run through every wave boundary of the image
    _check(oracle, gpu_ctx, masks)


@pytest.mark.parametrize("h,w", [(1, 200), (200, 1)])
def test_one_pixel_wide_images(oracle, gpu_ctx, h, w):
    _check(oracle, gpu_ctx, _random(3, h, w, seed=h))


def _staircases():
    """Image 0: x falls as y grows (each pixel joins up-right, the pixel above is clear); image 1: x grows (up-left)."""
    m = np.zeros((2, 9, 130), np.uint8)
    for k in range(5):
        m[0, 2 + k, 66 - k] = 1
        m[1, 2 + k, 62 + k] = 1
    m[:, 0, 3] = 1                                                  # a one-pixel component of its own, first in raster order
    return m


def test_diagonal_staircases_are_one_component(oracle, gpu_ctx):
    m = _staircases()
    for i in range(2):
        assert m[i, 2:7, 62:67].sum() == 5 and (m[i, 2:7, 62:67].sum(0) == 1).all() and (m[i, 2:7, 62:67].sum(1) == 1).all()
        want = oracle.clean_mask(m[i], 0.0, True)                   # the largest 8-component: a whole staircase
        assert want[2:7, 62:67].sum() == 5 and want[0, 3] == 0
    assert m[0, 2, 66] == 1 and m[1, 2, 62] == 1                    # anti-diagonal in image 0, main diagonal in image 1
    _check(oracle, gpu_ctx, m)


def _comb(h, w):
    m = np.zeros((1, h, w), np.uint8)
    m[0, 1, 1:w - 1] = 1                                            # the back
    m[0, 2:h - 2, 1:w - 1:2] = 1                                    # teeth, one pixel apart
    m[0, 2, 1:w - 1] = 1                                            # second row full: left, up and up-right all set
    m[0, h - 1, w - 1] = 1                                          # a separate pixel
    return m


def test_comb_is_one_component(oracle, gpu_ctx):
    m = _comb(12, 131)
    want = oracle.clean_mask(m[0], 0.0, True)
    assert np.array_equal(want[:11], m[0, :11]) and want[11, 130] == 0
    _check(oracle, gpu_ctx, m)


def test_equal_areas_keep_the_first_in_raster_order(oracle, gpu_ctx):
    m = np.zeros((2, 20, 70), np.uint8)
    m[0, 3:6, 60:66] = 1; m[0, 12:18, 2:5] = 1                      # 18 pixels each; the first spans the wave boundary
    m[1, 10:13, 2:8] = 1; m[1, 4:10, 66:69] = 1                     # the first in raster order is the one further right
    want0, want1 = oracle.clean_mask(m[0], 0.0, True), oracle.clean_mask(m[1], 0.0, True)
    assert want0.sum() == 18 and want0[3:6, 60:66].all()
    assert want1.sum() == 18 and want1[4:10, 66:69].all()
    _check(oracle, gpu_ctx, m)
