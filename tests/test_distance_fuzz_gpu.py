"""One fixed-seed pass of about 150 random cases through ggc_mask_distance and ggc_modify_mask against
tests/distance_ref.py: shapes weighted towards the wave and block boundaries, every mask kind plus rectangles and blobs,
random flag, cap, op and radii."""
import numpy as np
import pytest
import torch

import distance_cases as cases
import distance_ref as ref

pytestmark = pytest.mark.gpu
PARTS, CASES_PER_PART = 3, 50             # about 150 cases in all; a part keeps its reference to a couple of seconds
EDGES = (63, 64, 65, 127, 128, 129)


def draw_size(rng, top):
    edges = [e for e in EDGES if e <= top]
    return int(rng.choice(edges)) if rng.random() < 0.4 else int(rng.integers(1, top + 1))


@pytest.mark.parametrize("part", range(PARTS))
def test_random_cases_equal_the_reference(part):
    from gcn_grabcut._engine import get_engine
    eng = get_engine("cuda")
    rng = np.random.default_rng(20250 + part)
    for case in range(CASES_PER_PART):
        h, w, b = draw_size(rng, 70), draw_size(rng, 200), int(rng.integers(1, 5))
        masks = np.stack([cases.fuzz_mask(rng, h, w) for _ in range(b)])
        border = bool(rng.integers(0, 2))
        cap = int(rng.choice([0, 0, 1, 2, 5, 25, 26, 400, int(rng.integers(1, 5000)), 2 ** 29, 2 ** 40]))
        op = int(rng.integers(0, 6))
        r2_a = int(rng.choice([0, 1, 2, 4, 5, 9, 25, 100, int(rng.integers(0, 150))]))
        r2_b = int(rng.choice([0, 1, 2, 8, 9, 64, int(rng.integers(0, 150))])) if op in (ref.BORDER, ref.TRIMAP) else 0
        what = (part, case, h, w, b, border, cap, op, r2_a, r2_b)
        dev = eng.to_device(masks)
        d2 = torch.zeros((b, h, w), dtype=torch.int32, device="cuda")
        eng.ctx.call("ggc_mask_distance", eng._stream(), b, h, w, dev.data_ptr(), int(border), cap, d2.data_ptr())
        out = torch.full((b, h, w), 99, dtype=torch.uint8, device="cuda")
        eng.ctx.call("ggc_modify_mask", eng._stream(), b, h, w, dev.data_ptr(), op, r2_a, r2_b, int(border), out.data_ptr())
        assert np.array_equal(d2.cpu().numpy(), ref.signed_d2_batch(masks, border, cap)), what
        assert np.array_equal(out.cpu().numpy(), ref.modify_batch(masks, op, r2_a, r2_b, border)), what
