"""One fixed-seed pass of random magic-wand calls on the MI355X against tests/wand_ref.py, bit for bit: sizes around the
wave width, small batches, a few seeds per image (some outside), images quantised to a few levels per channel so that the
components are non-trivial, random options.  Every case is compared; none is skipped."""
import numpy as np
import pytest

import wand_cases as cases
import wand_ref as ref
from test_wand_gpu import call, label_mask

pytestmark = pytest.mark.gpu
N_CASES = 40


def side(rng):
    """1..70, biased to 63..65."""
    return int(rng.integers(63, 66)) if rng.random() < 0.4 else int(rng.integers(1, 71))


def draw(rng):
    h, w, b = side(rng), side(rng), int(rng.integers(1, 5))
    levels = int(rng.integers(2, 7))
    imgs = np.stack([cases.quantised(rng, h, w, levels) for _ in range(b)])
    per_image = []
    for _ in range(b):
        seeds = []
        for _ in range(int(rng.integers(0, 7))):
            r, c = int(rng.integers(-1, h + 1)), int(rng.integers(-1, w + 1))      # now and then outside the image
            seeds.append((r, c, int(rng.integers(0, 3))))                           # label 2 is foreground too
        per_image.append(seeds)
    step = 255 // (levels - 1)
    tol = int(rng.choice([0, 1, step - 1, step, step + 1, 2 * step, 254, 255]))
    return imgs, per_image, min(tol, 255), int(rng.choice([4, 8, 0])), int(rng.choice([1, 3, 5]))


def test_random_cases_equal_the_reference():
    from gcn_grabcut._engine import get_engine
    eng = get_engine("cuda")
    rng = np.random.default_rng(20240)
    compared = 0
    for k in range(N_CASES):
        imgs, per_image, tol, conn, sample = draw(rng)
        seeds, ptr = cases.pack(per_image)
        mask = label_mask(*imgs.shape[:3], seed=k)
        want = ref.wand_batch(imgs, seeds, ptr, tol, conn, sample, mask)
        got = call(eng, imgs, seeds, ptr, tol, conn, sample, mask)
        if len(seeds) == 0:                                                         # a no-op: the poisoned outputs come back
            assert np.array_equal(got[0], mask) and (got[1] == 7).all() and (got[2] == -5).all(), k
        else:
            for name, g, w in zip(("mask", "select", "counts"), got, want):
                assert np.array_equal(g, w), (k, name, imgs.shape, tol, conn, sample, per_image)
        compared += 1
    assert compared == N_CASES
