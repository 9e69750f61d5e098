"""A fixed-seed fuzz pass over ggc_mask_outlines: 40 cases, each a batch of random masks and of their 3x3-dilated versions
(smooth blobs with long straight runs), at shapes around the wave and tile sizes, against tests/outlines_ref.py, all five
arrays element for element."""
import numpy as np
import pytest

import outlines_ref as ref

pytestmark = pytest.mark.gpu
SIZES = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 70)
DENSITIES = (0.05, 0.3, 0.5, 0.7, 0.95)
N_CASES = 40
NAMES = ("verts", "loop_ptr", "loop_info", "image_ptr", "image_vert_ptr")


def dilate3(m):
    p = np.pad(m, ((0, 0), (1, 1), (1, 1)))
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[:, dy:dy + m.shape[1], dx:dx + m.shape[2]]
    return out


def case(i):
    rng = np.random.default_rng(7000 + i)
    h, w = int(rng.choice(SIZES)), int(rng.choice(SIZES))
    b = int(rng.integers(1, 6))
    density = DENSITIES[i % len(DENSITIES)]                             # every density 8 times
    conn = (4, 8)[(i // len(DENSITIES)) % 2]
    m = (rng.random((b, h, w)) < density).astype(np.uint8) * rng.choice(np.array([1, 2, 255], np.uint8), (b, h, w))
    sparse = (rng.random((b, h, w)) < density * 0.1).astype(np.uint8)   # the dilated masks start sparser: blobs, not a full image
    return h, w, b, density, conn, m, dilate3(sparse)


@pytest.fixture(scope="module")
def eng():
    from gcn_grabcut._engine import get_engine
    return get_engine("cuda")


@pytest.mark.parametrize("i", range(N_CASES))
def test_fuzz_case(eng, i):
    h, w, b, density, conn, m, blobs = case(i)
    for what, masks in (("random", m), ("dilated", blobs), ("random, dilated", dilate3(m))):
        got = tuple(t.cpu().numpy() for t in eng.mask_outlines(eng.to_device(np.ascontiguousarray(masks)), conn))
        want = ref.trace_batch(masks, conn)
        for name, g, x in zip(NAMES, got, want):
            assert g.dtype == np.int32 and g.shape == x.shape and np.array_equal(g, x), (i, what, (b, h, w), density, conn, name)
