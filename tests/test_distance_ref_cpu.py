"""The reference of the distance transform (tests/distance_ref.py) against itself: the separable form against the loop over
all pixel pairs, against scipy where it is installed, and the disk dilations and erosions against thresholds of the
transform.  No device is needed."""
import numpy as np
import pytest

import distance_ref as ref


def random_masks(seed, n, hmax=12, wmax=12):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        h, w = int(rng.integers(1, hmax + 1)), int(rng.integers(1, wmax + 1))
        yield (rng.random((h, w)) < rng.choice([0.05, 0.3, 0.5, 0.9])).astype(np.uint8)


@pytest.mark.parametrize("border", [False, True])
def test_every_3x3_mask_equals_the_pair_loop(border):
    for bits in range(512):
        m = np.array([(bits >> i) & 1 for i in range(9)], np.uint8).reshape(3, 3)
        assert np.array_equal(ref.signed_d2(m, border), ref.signed_d2_brute(m, border)), (bits, border)


def test_random_masks_equal_the_pair_loop():
    for i, m in enumerate(random_masks(11, 40)):
        for border in (False, True):
            for cap in (0, 1, 2, 9):
                assert np.array_equal(ref.signed_d2(m, border, cap), ref.signed_d2_brute(m, border, cap)), (i, border, cap)


def test_never_zero_and_the_sign_is_the_mask():
    for m in random_masks(12, 20):
        for border in (False, True):
            d = ref.signed_d2(m, border)
            assert d.dtype == np.int32 and np.all(d != 0) and np.array_equal(d < 0, m != 0)


def test_far_and_the_border_bound():
    full = np.ones((5, 7), np.uint8)
    assert np.all(ref.signed_d2(full) == -ref.FAR)
    assert np.all(ref.signed_d2(np.zeros((5, 7), np.uint8), True) == ref.FAR)
    d = -ref.signed_d2(full, True).astype(np.int64)
    y, x = np.mgrid[0:5, 0:7]
    assert np.array_equal(d, np.minimum(np.minimum(y + 1, 5 - y), np.minimum(x + 1, 7 - x)) ** 2)


def test_agrees_with_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    for density in (0.02, 0.5, 0.97):
        m = (rng.random((40, 57)) < density).astype(np.uint8)
        d = ref.signed_d2(m).astype(np.int64)
        d_in = np.rint(ndimage.distance_transform_edt(m) ** 2).astype(np.int64)
        d_out = np.rint(ndimage.distance_transform_edt(1 - m) ** 2).astype(np.int64)
        assert np.array_equal(np.where(m != 0, -d, 0), d_in) and np.array_equal(np.where(m == 0, d, 0), d_out)


@pytest.mark.parametrize("border", [False, True])
def test_disk_modifiers_are_thresholds_of_the_transform(border):
    for i, m in enumerate(random_masks(13, 25)):
        d = ref.signed_d2(m, border).astype(np.int64)
        fg = m != 0
        for r2 in (0, 1, 2, 4, 5, 25):
            assert np.array_equal(ref.grow(m, r2) != 0, fg | (d <= r2)), (i, r2)
            assert np.array_equal(ref.shrink(m, r2, border) != 0, fg & (-d > r2)), (i, r2)
        for r2_a, r2_b in ((0, 9), (9, 0), (2, 5)):
            band = (fg & (-d <= r2_a)) | (~fg & (d <= r2_b))
            assert np.array_equal(ref.modify(m, ref.BORDER, r2_a, r2_b, border) != 0, band), (i, r2_a, r2_b)
            tri = np.where(fg & (-d > r2_a), 255, np.where(~fg & (d > r2_b), 0, 128))
            assert np.array_equal(ref.modify(m, ref.TRIMAP, r2_a, r2_b, border), tri), (i, r2_a, r2_b)


def test_shrink_is_the_dual_of_grow_without_the_border_flag():
    for m in random_masks(14, 25):
        for r2 in (0, 1, 2, 8, 16):
            assert np.array_equal(ref.shrink(m, r2), 1 - ref.grow(1 - m, r2))


def test_open_and_close_bracket_the_mask():
    for m in random_masks(15, 25):
        for r2 in (1, 2, 4):
            o, c = ref.modify(m, ref.OPEN, r2), ref.modify(m, ref.CLOSE, r2)
            assert np.all(o <= (m != 0)) and np.all((m != 0) <= c)
            assert np.array_equal(ref.modify(o, ref.OPEN, r2), o)
