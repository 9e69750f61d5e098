"""The exact distance transform on the MI355X: ggc_mask_distance through ctx.call against the numpy restatement of its
definition (tests/distance_ref.py), element for element: thin, odd and multi-block shapes, degenerate and worst-case masks,
both border flags, caps on both sides of a ring at d2 = 25, FAR, batch against single calls, refusals, the size limit."""
import numpy as np
import pytest
import torch

import distance_cases as cases
import distance_ref as ref

pytestmark = pytest.mark.gpu
POISON = -7


@pytest.fixture(scope="module")
def eng():
    from gcn_grabcut._engine import get_engine
    return get_engine("cuda")


def distance(eng, masks, border=False, cap=0):
    """One ggc_mask_distance call on a poisoned plane -> (B, H, W) int32 on the host."""
    masks = np.array(masks, dtype=np.uint8)                             # a writable copy: the shared masks are read-only
    b, h, w = masks.shape
    dev = eng.to_device(masks)
    out = torch.full((b, h, w), POISON, dtype=torch.int32, device="cuda")
    eng.ctx.call("ggc_mask_distance", eng._stream(), b, h, w, dev.data_ptr(), int(border), int(cap), out.data_ptr())
    return out.cpu().numpy()


@pytest.mark.parametrize("border", [False, True])
@pytest.mark.parametrize("shape", cases.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_mask_kind_and_cap_equals_the_reference(eng, shape, border):
    for kind in cases.KINDS:
        m = cases.mask(shape, kind)
        want = cases.unbounded(shape, kind, border)
        for cap in cases.CAPS:
            got = distance(eng, m[None], border, cap)[0]
            assert got.dtype == np.int32 and np.array_equal(got, ref.apply_cap(want, cap)), (shape, kind, border, cap)
            assert np.all(got != 0) and np.array_equal(got < 0, m != 0), (shape, kind, border, cap)      # never 0; sign -> mask


def test_far_is_where_the_reference_says(eng):
    shape = (33, 300)
    assert np.all(distance(eng, cases.mask(shape, "full")[None])[0] == -ref.FAR)             # no background anywhere
    assert np.all(distance(eng, cases.mask(shape, "empty")[None], True)[0] == ref.FAR)       # outside is never foreground
    d = -distance(eng, cases.mask(shape, "full")[None], True)[0].astype(np.int64)
    y, x = np.mgrid[0:33, 0:300]
    assert np.array_equal(d, np.minimum(np.minimum(y + 1, 33 - y), np.minimum(x + 1, 300 - x)) ** 2)
    got = distance(eng, cases.mask(shape, "dot_in_corner")[None], False, 25)[0]
    assert (np.abs(got) == ref.FAR).sum() == 33 * 300 - 1 - len([1 for dy in range(6) for dx in range(6) if 0 < dy * dy + dx * dx <= 25])


def test_the_ring_at_25_separates_le_from_lt(eng):
    shape = (64, 64)
    m = cases.mask(shape, "ring25")
    c = (32, 32)
    want = cases.unbounded(shape, "ring25", False)
    assert want[c] == 25
    for cap, value in ((24, ref.FAR), (25, 25), (26, 25), (0, 25)):
        got = distance(eng, m[None], False, cap)[0]
        assert got[c] == value and np.array_equal(got, ref.apply_cap(want, cap)), cap


@pytest.mark.parametrize("border", [False, True])
def test_batch_of_five_equals_its_single_calls(eng, border):
    shape = (33, 70)
    kinds = ("full", "empty", "noise_0.5", "two_disks", "hole_in_corner")
    masks = np.stack([cases.mask(shape, k) for k in kinds])
    for cap in (0, 26):
        got = distance(eng, masks, border, cap)
        for i, k in enumerate(kinds):
            assert np.array_equal(got[i], distance(eng, masks[i:i + 1], border, cap)[0]), (k, cap)
            assert np.array_equal(got[i], ref.apply_cap(cases.unbounded(shape, k, border), cap)), (k, cap)


def test_any_nonzero_byte_is_foreground(eng):
    shape = (7, 5)
    m = cases.mask(shape, "noise_0.5")
    bytes_ = m * np.random.default_rng(1).choice(np.array([1, 7, 128, 255], np.uint8), shape)
    assert np.array_equal(distance(eng, bytes_[None])[0], cases.unbounded(shape, "noise_0.5", False))


def test_refusals_leave_the_output_untouched(eng):
    from gcn_grabcut import _native
    mask = torch.ones(2, 4, 5, dtype=torch.uint8, device="cuda")
    d2 = torch.full((2, 4, 5), POISON, dtype=torch.int32, device="cuda")
    u8 = torch.full((2, 4, 5), 99, dtype=torch.uint8, device="cuda")
    ok = dict(B=2, H=4, W=5, mask=mask.data_ptr(), flags=0, cap=0, out=d2.data_ptr())
    cases_d = [(dict(H=0), -2), (dict(W=0), -2), (dict(H=16385), -2), (dict(W=16385), -2), (dict(H=-1), -2),
               (dict(B=8, H=16384, W=16384), -2), (dict(B=2 ** 31 - 1, H=2, W=1), -2),
               (dict(mask=None), -1), (dict(out=None), -1), (dict(flags=2), -1), (dict(flags=-1), -1), (dict(cap=-1), -1)]
    for change, code in cases_d:
        a = dict(ok, **change)
        with pytest.raises(_native.GGCError) as e:
            eng.ctx.call("ggc_mask_distance", eng._stream(), a["B"], a["H"], a["W"], a["mask"], a["flags"], a["cap"], a["out"])
        assert e.value.code == code, change
    ok = dict(B=2, H=4, W=5, mask=mask.data_ptr(), op=0, a=1, b=0, flags=0, out=u8.data_ptr())
    cases_m = [(dict(H=0), -2), (dict(W=16385), -2), (dict(B=8, H=16384, W=16384), -2), (dict(mask=None), -1),
               (dict(out=None), -1), (dict(flags=4), -1), (dict(op=6), -1), (dict(op=-1), -1), (dict(a=-1), -1),
               (dict(op=2, b=-1), -1)] + [(dict(op=op, b=1), -1) for op in (0, 1, 3, 4)]
    for change, code in cases_m:
        a = dict(ok, **change)
        with pytest.raises(_native.GGCError) as e:
            eng.ctx.call("ggc_modify_mask", eng._stream(), a["B"], a["H"], a["W"], a["mask"], a["op"], a["a"], a["b"], a["flags"], a["out"])
        assert e.value.code == code, change
    eng.ctx.call("ggc_mask_distance", eng._stream(), 0, 4, 5, None, 0, 0, None)                  # B == 0: a no-op
    eng.ctx.call("ggc_modify_mask", eng._stream(), 0, 4, 5, None, 0, 1, 0, 0, None)
    torch.cuda.synchronize()
    assert (d2 == POISON).all() and (u8 == 99).all() and (mask == 1).all()                       # refused before any launch


@pytest.mark.parametrize("shape", [(16384, 3), (3, 16384)], ids=["16384x3", "3x16384"])
def test_index_arithmetic_at_the_size_limit(eng, shape):
    """One strip of foreground near the far end; the reference is computed on windows at both ends and across the strip."""
    h, w = shape
    m = np.zeros(shape, np.uint8)
    if h > w:
        m[16000:16100, :] = 1
        windows = [(r, r + 64, 0, 3) for r in (0, 15968, 16068, h - 64)]
    else:
        m[:, 16000:16100] = 1
        windows = [(0, 3, c, c + 64) for c in (0, 15968, 16068, w - 64)]
    got = distance(eng, m[None])[0]
    assert np.all(got != 0) and np.array_equal(got < 0, m != 0)
    edge = distance(eng, m[None], True)[0]
    assert np.array_equal(edge < 0, m != 0)
    for r0, r1, c0, c1 in windows:
        want = ref.signed_d2_window(m, r0, r1, c0, c1)
        assert np.array_equal(got[r0:r1, c0:c1], want), (r0, c0)
        bg = m[r0:r1, c0:c1] == 0              # the reference's ring would be 16384 wide; the flag does not bear on the background
        assert np.array_equal(edge[r0:r1, c0:c1][bg], want[bg]), (r0, c0)
    got = distance(eng, m[None], False, 100)[0]
    r0, r1, c0, c1 = windows[1]
    assert np.array_equal(got[r0:r1, c0:c1], ref.signed_d2_window(m, r0, r1, c0, c1, False, 100))
