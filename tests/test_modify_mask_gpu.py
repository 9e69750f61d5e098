"""The mask modifiers on the MI355X: ggc_modify_mask against explicit disk dilations and erosions (tests/distance_ref.py),
aliasing, input bytes, the algebra of the ops on device results, and the public functions on top."""
import numpy as np
import pytest
import torch

import distance_cases as cases
import distance_ref as ref
from helpers import seeded_state_dict

pytestmark = pytest.mark.gpu
SHAPES = cases.SHAPES                   # the shapes and masks of tests/test_distance_gpu.py
R2 = (0, 1, 2, 4, 25, 100)
PAIRS = [(r, r) for r in R2] + [(0, 9), (9, 0), (2, 25)]


@pytest.fixture(scope="module")
def eng():
    from gcn_grabcut._engine import get_engine
    return get_engine("cuda")


def modify(eng, masks, op, r2_a, r2_b=0, border=False, alias=False):
    """One ggc_modify_mask call -> (B, H, W) uint8 on the host; alias: out is mask_in."""
    masks = np.array(masks, dtype=np.uint8)                             # a writable copy: the shared masks are read-only
    b, h, w = masks.shape
    dev = eng.to_device(masks)
    out = dev if alias else torch.full((b, h, w), 99, dtype=torch.uint8, device="cuda")
    eng.ctx.call("ggc_modify_mask", eng._stream(), b, h, w, dev.data_ptr(), int(op), int(r2_a), int(r2_b), int(border), out.data_ptr())
    return out.cpu().numpy()


def radii(op):
    return PAIRS if op in (ref.BORDER, ref.TRIMAP) else [(r, 0) for r in R2]


@pytest.mark.parametrize("border", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_op_and_radius_equals_the_disk_reference(eng, shape, border):
    masks = np.stack([cases.mask(shape, k) for k in cases.KINDS])         # one batch per call, one image per mask kind
    for op in range(6):
        for r2_a, r2_b in radii(op):
            got = modify(eng, masks, op, r2_a, r2_b, border)
            want = ref.modify_batch(masks, op, r2_a, r2_b, border)
            for i, kind in enumerate(cases.KINDS):
                assert np.array_equal(got[i], want[i]), (shape, kind, border, op, r2_a, r2_b)


def test_zero_radius_is_the_identity_and_an_empty_border(eng):
    m = cases.mask((33, 300), "noise_0.5") * np.uint8(255)
    for op in (ref.GROW, ref.SHRINK, ref.OPEN, ref.CLOSE):
        assert np.array_equal(modify(eng, m[None], op, 0)[0], (m != 0).astype(np.uint8))       # normalised to {0, 1}
    assert not modify(eng, m[None], ref.BORDER, 0, 0).any()


@pytest.mark.parametrize("border", [False, True])
def test_out_may_alias_the_input(eng, border):
    masks = np.stack([cases.mask((33, 300), k) for k in ("noise_0.5", "two_disks", "frame", "noise_0.99")])
    for op in range(6):
        r2_a, r2_b = (4, 9) if op in (ref.BORDER, ref.TRIMAP) else (4, 0)
        assert np.array_equal(modify(eng, masks, op, r2_a, r2_b, border, alias=True), ref.modify_batch(masks, op, r2_a, r2_b, border)), op


def test_any_nonzero_byte_is_foreground(eng):
    m = cases.mask((64, 64), "two_disks")
    bytes_ = m * np.random.default_rng(2).choice(np.array([1, 7, 255], np.uint8), m.shape)
    for op in range(6):
        r2_a, r2_b = (5, 2) if op in (ref.BORDER, ref.TRIMAP) else (5, 0)
        assert np.array_equal(modify(eng, bytes_[None], op, r2_a, r2_b)[0], ref.modify(m, op, r2_a, r2_b)), op


@pytest.mark.parametrize("border", [False, True])
def test_algebra_of_the_ops_on_device_results(eng, border):
    masks = np.stack([cases.mask((65, 129), k) for k in ("noise_0.5", "noise_0.99", "two_disks", "checkerboard", "frame")])
    fg = masks != 0
    for r2 in (1, 2, 9):
        opened, closed = modify(eng, masks, ref.OPEN, r2, 0, border), modify(eng, masks, ref.CLOSE, r2, 0, border)
        assert np.all(opened <= fg)                                                           # open in mask ...
        assert border or np.all(fg <= closed)             # ... in close; with the flag the closing's shrink eats from the edge
        assert np.array_equal(modify(eng, opened, ref.OPEN, r2, 0, border), opened)           # open is idempotent
    for r2_a, r2_b in ((4, 4), (0, 9), (9, 0), (2, 25)):
        grown, shrunk = modify(eng, masks, ref.GROW, r2_b), modify(eng, masks, ref.SHRINK, r2_a, 0, border)
        assert np.array_equal(modify(eng, masks, ref.BORDER, r2_a, r2_b, border), grown & (1 - shrunk))
        tri = modify(eng, masks, ref.TRIMAP, r2_a, r2_b, border)
        assert set(np.unique(tri)) <= {0, 128, 255}
        assert np.array_equal(tri == 255, shrunk != 0) and np.array_equal(tri != 0, grown != 0)


# ---------------------------------------------------------------- the public functions

def test_mask_distance_as_floats(eng):
    import gcn_grabcut as g
    m = cases.mask((33, 300), "two_disks")
    want = cases.unbounded((33, 300), "two_disks", False).astype(np.int64)
    d = g.mask_distance(m)
    assert d.dtype == np.float64 and np.array_equal(d, np.sign(want) * np.sqrt(np.abs(want)))
    assert np.array_equal(g.mask_distance(m, signed=False), np.sqrt(np.abs(want)))
    assert np.array_equal(g.mask_distance(m, squared=True), want.astype(np.int32))
    capped = g.mask_distance(m, max_distance=5)                                               # d2 <= 25 stays, the rest is inf
    assert np.array_equal(capped, np.where(np.abs(want) <= 25, np.sign(want) * np.sqrt(np.abs(want)), np.sign(want) * np.inf))
    full = np.ones((7, 5), np.uint8)
    assert np.all(g.mask_distance(full) == -np.inf) and np.all(g.mask_distance(1 - full, signed=False) == np.inf)
    assert np.array_equal(g.mask_distance(full, squared=True, border_background=True), ref.signed_d2(full, True))
    both = g.mask_distance_batch(np.stack([m, 1 - m]), squared=True, border_background=True)
    assert np.array_equal(both[0], cases.unbounded((33, 300), "two_disks", True)) and np.array_equal(both[1], ref.signed_d2(1 - m, True))


def test_public_modifiers_and_chained_steps():
    import gcn_grabcut as g
    m = cases.mask((33, 300), "noise_0.99")
    assert np.array_equal(g.grow_mask(m, 2), ref.grow(m, 4)) and np.array_equal(g.grow_mask(m, radius2=2), ref.grow(m, 2))
    assert np.array_equal(g.shrink_mask(m, 1.5), ref.shrink(m, 2))
    assert np.array_equal(g.shrink_mask(m, 1.5, border_background=True), ref.shrink(m, 2, True))
    assert np.array_equal(g.open_mask(m, 2), ref.modify(m, ref.OPEN, 4)) and np.array_equal(g.close_mask(m, 2), ref.modify(m, ref.CLOSE, 4))
    assert np.array_equal(g.border_mask(m, 2), ref.modify(m, ref.BORDER, 4, 4))
    assert np.array_equal(g.border_mask(m, 1, 3), ref.modify(m, ref.BORDER, 1, 9))
    assert np.array_equal(g.mask_to_trimap(m, 2, 3), ref.modify(m, ref.TRIMAP, 4, 9))
    assert np.array_equal(g.mask_to_trimap(m, radius2=(5, 0)), ref.modify(m, ref.TRIMAP, 5, 0))
    steps = (g.ModifyMask("shrink", 2, border_background=True), g.ModifyMask("grow", 3), g.ModifyMask("border", 1, 2))
    chained = g.modify_mask(m, *steps)
    one_by_one = m
    for s in steps:
        one_by_one = g.modify_mask(one_by_one, s)
    assert np.array_equal(chained, one_by_one)
    assert np.array_equal(chained, ref.modify(ref.grow(ref.shrink(m, 4, True), 9), ref.BORDER, 1, 4))
    batch = g.modify_mask_batch(np.stack([m, 1 - m]), *steps)
    assert np.array_equal(batch[0], chained) and np.array_equal(batch[1], g.modify_mask(1 - m, *steps))


def test_result_methods_on_a_lasso_cut():
    from gcn_grabcut import GCNGrabCutPipeline, ModifyMask, SuperpixelGraphConfig
    from gcn_grabcut.synthetic import synthetic_image
    model, _ = seeded_state_dict(32, 2, seed=5)
    pipe = GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=80), device="cuda")
    img = synthetic_image(60, 80, 30001)
    ctx = pipe._eng.ctx
    ctx.profile_enable(1)
    try:
        res = pipe.segment_lasso(img, [(5, 8), (5, 72), (55, 72), (55, 8)])
        assert [ctx.profile_query(n)[0] for n in ("distance_cols", "distance_rows")] == [0, 0]      # a plain run launches neither
        got = res.modified(ModifyMask("shrink", 2), ModifyMask("grow", 2))
        assert [ctx.profile_query(n)[0] for n in ("distance_cols", "distance_rows")] == [2, 2]
    finally:
        ctx.profile_enable(0)
    m = res.binary_mask
    assert m.any() and np.array_equal(got, ref.modify(m, ref.OPEN, 4))
    assert np.array_equal(res.trimap_from_mask(2, 4), ref.modify(m, ref.TRIMAP, 4, 16))
    assert np.array_equal(res.trimap_from_mask(3), ref.modify(m, ref.TRIMAP, 9, 9))


def test_a_mask_reaches_the_trimap_matte():
    import gcn_grabcut as g
    from gcn_grabcut.synthetic import synthetic_image
    img, gt = synthetic_image(48, 64, 30002, return_mask=True)
    tri = g.mask_to_trimap(gt, 3, 5)
    assert np.array_equal(tri, ref.modify(gt, ref.TRIMAP, 9, 25)) and {0, 128, 255} >= set(np.unique(tri))
    alpha = g.trimap_matte(img, tri)
    assert alpha.shape == (48, 64) and np.all(alpha[tri == 255] == 1) and np.all(alpha[tri == 0] == 0)
    assert np.all((alpha >= 0) & (alpha <= 1))
