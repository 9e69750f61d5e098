"""Mask outlines on the MI355X: ggc_mask_outlines against the integer restatement of its definition (tests/outlines_ref.py),
all five output arrays element for element; then the painter fed with a traced batch, the count-only call, capacities,
refusals, SegmentationResult.outlines and the command line's --save outlines."""
import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import geodesic_ref
import outlines_ref as ref
import polygons_ref
from helpers import seeded_state_dict

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
POISON = -7
NAMES = ("verts", "loop_ptr", "loop_info", "image_ptr", "image_vert_ptr")
SCOPES = ("outline_mark", "outline_scan", "outline_fill", "outline_jump", "outline_loops", "outline_label", "outline_emit")
H0, W0 = 37, 53      # no multiple of a 32x8 tile or of a 64-pixel wave


@pytest.fixture(scope="module")
def eng():
    from gcn_grabcut._engine import get_engine
    return get_engine("cuda")


def trace(eng, masks, connectivity):
    """(B, H, W) uint8 -> the five arrays on the host, through Engine.mask_outlines (a counting and a filling call)."""
    out = eng.mask_outlines(eng.to_device(np.ascontiguousarray(masks, dtype=np.uint8)), connectivity)
    return tuple(t.cpu().numpy() for t in out)


def assert_same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (what, name)


def check(eng, masks, connectivity, what=""):
    masks = np.ascontiguousarray(masks, dtype=np.uint8)
    got = trace(eng, masks, connectivity)
    assert_same(got, ref.trace_batch(masks, connectivity), (what, connectivity))
    return got


def raw(eng, masks, connectivity, loop_capacity=None, vert_capacity=None):
    """One ggc_mask_outlines call on poisoned arrays of the given capacities (None: no fill arrays) -> the five tensors."""
    b, h, w = masks.shape
    dev = eng.to_device(masks)
    ip = torch.full((b + 1,), POISON, dtype=torch.int32, device="cuda")
    ivp = torch.full((b + 1,), POISON, dtype=torch.int32, device="cuda")
    if loop_capacity is None:
        eng.ctx.call("ggc_mask_outlines", eng._stream(), b, h, w, dev.data_ptr(), connectivity, ip.data_ptr(), ivp.data_ptr(),
                     None, None, None, 0, 0)
        return None, None, None, ip, ivp
    lp = torch.full((loop_capacity + 1,), POISON, dtype=torch.int32, device="cuda")
    li = torch.full((loop_capacity, 3), POISON, dtype=torch.int32, device="cuda")
    v = torch.full((vert_capacity, 2), POISON, dtype=torch.int32, device="cuda")
    out = (v, lp, li, ip, ivp)
    try:
        eng.ctx.call("ggc_mask_outlines", eng._stream(), b, h, w, dev.data_ptr(), connectivity, ip.data_ptr(), ivp.data_ptr(),
                     lp.data_ptr(), li.data_ptr(), v.data_ptr(), loop_capacity, vert_capacity)
    except Exception as e:
        e.outputs = out
        raise
    return out


@functools.lru_cache(maxsize=None)
def kernel_masks():
    """B = 4 at 37x53: random, empty, full, checkerboard; the set values are 1 and 255 mixed."""
    rng = np.random.default_rng(3)
    m = np.zeros((4, H0, W0), np.uint8)
    m[0] = rng.random((H0, W0)) < 0.5
    m[2] = 1
    m[3] = np.add.outer(np.arange(H0), np.arange(W0)) % 2 == 0
    m *= rng.choice(np.array([1, 255], np.uint8), m.shape)
    return m


# ---------------------------------------------------------------- against the reference

@pytest.mark.parametrize("connectivity", [4, 8])
def test_batch_of_four_and_its_single_images(eng, connectivity):
    masks = kernel_masks()
    got = check(eng, masks, connectivity, "batch")
    assert got[3].tolist()[1:3] == [got[3][1]] * 2                      # the empty image owns no loop
    for b in range(4):
        one = trace(eng, masks[b:b + 1], connectivity)
        assert_same(one, ref.trace_batch(masks[b:b + 1], connectivity), ("single", b))
        lo, hi = got[3][b], got[3][b + 1]
        vlo, vhi = got[4][b], got[4][b + 1]
        assert np.array_equal(one[0], got[0][vlo:vhi]) and np.array_equal(one[2], got[2][lo:hi])
        assert np.array_equal(one[1], got[1][lo:hi + 1] - vlo)


@pytest.mark.parametrize("shape", [(64, 64), (33, 65)])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_outline_through_every_tile_corner(eng, shape, connectivity):
    h, w = shape
    tiles = (np.add.outer(np.arange(h) // 8, np.arange(w) // 32) % 2 == 0).astype(np.uint8)     # a saddle at every tile corner
    blob = np.zeros(shape, np.uint8)
    blob[3:h - 2, 5:w - 7] = 1
    blob[::8, :] = 0                                                    # cut along every tile row ...
    blob[:, 31:w:32] = 0                                                # ... and beside every tile column
    blob[4::8, :] |= tiles[4::8, :]
    check(eng, np.stack([tiles, blob]), connectivity, shape)


@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (70, 1)])
def test_thin_images(eng, shape):
    rng = np.random.default_rng(shape[1])
    for conn in (4, 8):
        check(eng, np.stack([np.ones(shape), np.zeros(shape), rng.random(shape) < 0.6]), conn, shape)


@pytest.mark.parametrize("width", [31, 32, 127, 128, 511, 512])
def test_loops_either_side_of_a_doubling_round(eng, width):
    """A set 1 x W strip is one loop of 2 W + 2 cracks: 64, 256, 1024 take exactly 6, 8, 10 rounds, 66, 258, 1026 one more."""
    got = check(eng, np.ones((1, 1, width), np.uint8), 8, width)
    assert got[2].tolist() == [[width, 0, 2 * width + 2]]
    assert got[0].tolist() == [[0, 0], [0, width], [1, width], [1, 0]]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_serpentine(eng, connectivity):
    """The corridor between geodesic_ref.serpentine's walls is one component whose outline runs through every tile of the
    70x70 frame; the walls are the loops beside it.  Alone and as image 2 of 3."""
    walls = (geodesic_ref.serpentine()[:, :, 0] == 20).astype(np.uint8)
    corridor = 1 - walls
    alone = check(eng, corridor[None], connectivity, "corridor")
    assert alone[2].shape == (1, 3) and alone[2][0, 2] > 1500           # one loop of thousands of cracks
    check(eng, walls[None], connectivity, "walls")
    rng = np.random.default_rng(1)
    three = check(eng, np.stack([walls, (rng.random((70, 70)) < 0.4).astype(np.uint8), corridor]), connectivity, "image 2 of 3")
    assert np.array_equal(three[0][three[4][2]:], alone[0]) and np.array_equal(three[2][three[3][2]:], alone[2])


def nested_rings():
    m = np.zeros((15, 17), np.uint8)
    for k in (0, 2, 4):
        m[k:15 - k, k:17 - k] = 1
        m[k + 1:14 - k, k + 1:16 - k] = 0
    m[7, 8] = 1
    return m


@pytest.mark.parametrize("connectivity", [4, 8])
def test_rings_nested_three_deep(eng, connectivity):
    m = nested_rings()
    got = check(eng, np.stack([np.zeros_like(m), m]), connectivity, "rings")
    area, outer = got[2][:, 0].tolist(), got[2][:, 1].tolist()
    assert [a > 0 for a in area] == [True, False, True, False, True, False, True]
    assert outer == [0, 0, 2, 2, 4, 4, 6]                               # every hole names the ring around it


def test_hole_touching_the_outer_loop_at_a_saddle(eng):
    m = np.ones((9, 9), np.uint8)
    m[3:6, 3:6] = 0
    m[6:, 6:] = 0                                                       # the hole's corner (6, 6) meets the outside
    m2 = np.array([[1, 1, 1], [1, 0, 1], [1, 1, 0]], np.uint8)
    for conn in (4, 8):
        check(eng, m[None], conn, "saddle 9x9")
        got = check(eng, m2[None], conn, "saddle 3x3")
        assert got[2].tolist() == ([[8, 0, 12], [-1, 0, 4]] if conn == 8 else [[7, 0, 16]])


# ---------------------------------------------------------------- the painter fills the loops back

def test_round_trip_through_the_polygon_painter(eng):
    """The traced batch, doubled, goes to ggc_apply_polygons loop by loop on the (2H+1) x (2W+1) grid without leaving the
    device: one loop per image of a batch of Q.  The XOR of an image's fills, at the odd positions, is its mask."""
    rng = np.random.default_rng(9)
    h, w = 21, 30
    masks = np.stack([np.pad(nested_rings(), ((3, 3), (6, 7)))] + [(rng.random((h, w)) < d).astype(np.uint8) for d in (0.2, 0.6)])
    assert masks.shape == (3, h, w)
    for conn in (4, 8):
        verts, loop_ptr, info, image_ptr, _ = eng.mask_outlines(eng.to_device(masks), conn)
        q = int(info.shape[0])
        grid = torch.zeros(q, 2 * h + 1, 2 * w + 1, dtype=torch.uint8, device="cuda")
        label = torch.ones(q, dtype=torch.int32, device="cuda")                        # a foreground fill each
        eng.apply_polygons(grid, (verts * 2).contiguous(), loop_ptr, label, torch.arange(q + 1, dtype=torch.int32, device="cuda"))
        fills = grid[:, 1::2, 1::2].cpu().numpy()
        assert set(np.unique(fills)) <= {0, 1}
        ip = image_ptr.cpu().numpy()
        for b in range(3):
            back = np.bitwise_xor.reduce(fills[ip[b]:ip[b + 1]], axis=0) if ip[b + 1] > ip[b] else np.zeros((h, w), np.uint8)
            assert np.array_equal(back, masks[b]), (conn, b)


# ---------------------------------------------------------------- the entry's contract

def test_count_only_call(eng):
    masks = kernel_masks()
    for conn in (4, 8):
        want = ref.trace_batch(masks, conn)
        _, _, _, ip, ivp = raw(eng, masks, conn)
        assert np.array_equal(ip.cpu().numpy(), want[3]) and np.array_equal(ivp.cpu().numpy(), want[4])


def test_capacity_one_too_small_keeps_the_poison(eng):
    from gcn_grabcut import _native
    masks = kernel_masks()
    want = ref.trace_batch(masks, 8)
    q, v = int(want[3][-1]), int(want[4][-1])
    for lc, vc in ((q - 1, v), (q, v - 1)):
        with pytest.raises(_native.GGCError, match="INVALID_ARG") as e:
            raw(eng, masks, 8, lc, vc)
        assert e.value.code == -1
        verts, lp, li, ip, ivp = e.value.outputs
        assert (verts == POISON).all() and (lp == POISON).all() and (li == POISON).all()        # nothing written
        assert np.array_equal(ip.cpu().numpy(), want[3]) and np.array_equal(ivp.cpu().numpy(), want[4])
    got = raw(eng, masks, 8, q + 3, v + 5)                              # room to spare: the rest keeps its poison
    assert_same((got[0][:v].cpu().numpy(), got[1][:q + 1].cpu().numpy(), got[2][:q].cpu().numpy(), got[3].cpu().numpy(),
                 got[4].cpu().numpy()), want)
    assert (got[0][v:] == POISON).all() and (got[1][q + 1:] == POISON).all() and (got[2][q:] == POISON).all()


def test_refusals(eng):
    from gcn_grabcut import _native
    m = torch.ones(2, 4, 5, dtype=torch.uint8, device="cuda")
    ip = torch.full((3,), POISON, dtype=torch.int32, device="cuda")
    ivp = torch.full((3,), POISON, dtype=torch.int32, device="cuda")
    lp = torch.full((9,), POISON, dtype=torch.int32, device="cuda")
    li = torch.full((8, 3), POISON, dtype=torch.int32, device="cuda")
    v = torch.full((32, 2), POISON, dtype=torch.int32, device="cuda")
    P = lambda t: None if t is None else t.data_ptr()
    ok = dict(B=2, H=4, W=5, mask=m, conn=8, ip=ip, ivp=ivp, lp=lp, li=li, v=v, lc=8, vc=32)
    cases = [(dict(H=0), -2), (dict(W=0), -2), (dict(H=65536), -2), (dict(W=65536), -2), (dict(B=-1), -2), (dict(B=65536), -2),
             (dict(H=16384, W=16384), -1),                              # 16385^2 corners > 2^28
             (dict(conn=6), -1), (dict(conn=0), -1), (dict(mask=None), -1), (dict(ip=None), -1), (dict(ivp=None), -1),
             (dict(lp=None), -1), (dict(li=None), -1), (dict(v=None), -1), (dict(lp=None, li=None), -1),
             (dict(lc=-1), -1), (dict(vc=-1), -1)]
    for change, code in cases:
        a = dict(ok, **change)
        with pytest.raises(_native.GGCError) as e:
            eng.ctx.call("ggc_mask_outlines", eng._stream(), a["B"], a["H"], a["W"], P(a["mask"]), a["conn"], P(a["ip"]), P(a["ivp"]),
                         P(a["lp"]), P(a["li"]), P(a["v"]), a["lc"], a["vc"])
        assert e.value.code == code, change
    torch.cuda.synchronize()
    for t in (ip, ivp, lp, li, v):
        assert (t == POISON).all()                                      # refused before any launch
    eng.ctx.call("ggc_mask_outlines", eng._stream(), 0, 4, 5, P(m), 8, P(ip), P(ivp), P(lp), P(li), P(v), 8, 32)   # B == 0: a no-op
    torch.cuda.synchronize()
    for t in (ip, ivp, lp, li, v):
        assert (t == POISON).all()
    eng.ctx.call("ggc_mask_outlines", eng._stream(), 2, 4, 5, P(m), 8, P(ip), P(ivp), P(lp), P(li), P(v), 8, 32)
    assert ip.tolist() == [0, 1, 2] and ivp.tolist() == [0, 4, 8] and lp.tolist()[:3] == [0, 4, 8]
    assert li.tolist()[:2] == [[20, 0, 18], [20, 0, 18]]


def test_empty_batch_through_the_engine(eng):
    out = eng.mask_outlines(torch.zeros(0, 4, 5, dtype=torch.uint8, device="cuda"), 8)
    assert [tuple(t.shape) for t in out] == [(0, 2), (1,), (0, 3), (1,), (1,)] and int(out[1][0]) == 0 and int(out[3][0]) == 0
    out = eng.mask_outlines(torch.zeros(3, 4, 5, dtype=torch.uint8, device="cuda"), 4)
    assert [tuple(t.shape) for t in out] == [(0, 2), (1,), (0, 3), (4,), (4,)] and not out[3].any() and not out[4].any()


def test_engine_capacity_guess(eng):
    masks = kernel_masks()
    want = ref.trace_batch(masks, 8)
    q, v = int(want[3][-1]), int(want[4][-1])
    dev = eng.to_device(masks)
    for guess in ((q, v), (q + 10, v + 100), (q - 1, v), (q, v - 1), (0, 0)):      # exact, ample, short: the call is repeated
        assert_same(tuple(t.cpu().numpy() for t in eng.mask_outlines(dev, 8, capacity=guess)), want, guess)
    none = eng.mask_outlines(torch.zeros(2, 5, 6, dtype=torch.uint8, device="cuda"), 8, capacity=(4, 16))
    assert [tuple(t.shape) for t in none] == [(0, 2), (1,), (0, 3), (3,), (3,)]
    from gcn_grabcut import _native
    with pytest.raises(_native.GGCError, match="connectivity"):         # refused for another reason: not repeated
        eng.mask_outlines(dev, 5, capacity=(q, v))


def test_two_runs_give_identical_bytes(eng):
    rng = np.random.default_rng(21)
    masks = (rng.random((6, 65, 70)) < 0.55).astype(np.uint8)
    first = trace(eng, masks, 8)
    eng.mask_outlines(eng.to_device(kernel_masks()), 4)                 # other work in the same scratch in between
    second = trace(eng, masks, 8)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


def test_image_groups_give_the_results_of_the_single_images(eng):
    """A batch of more than 2^26 corners is worked through in image groups: three sparse 4097 x 5501 images go as two groups
    (2 + 1).  Every image's part of the batch equals its single-image call."""
    h, w = 4097, 5501
    rng = np.random.default_rng(2)
    masks = np.zeros((3, h, w), np.uint8)
    for b in range(3):
        for _ in range(6):
            y, x = int(rng.integers(0, h - 300)), int(rng.integers(0, w - 300))
            masks[b, y:y + int(rng.integers(2, 300)), x:x + int(rng.integers(2, 300))] ^= 1
        y, x = int(rng.integers(0, h - 64)), int(rng.integers(0, w - 64))
        masks[b, y:y + 64, x:x + 64] = rng.random((64, 64)) < 0.5
    masks[0, 0, 0] = masks[0, -1, -1] = masks[1, -1, 0] = masks[2, 0, -1] = 1
    masks[2, h // 2] = 1                                                # a loop as wide as the image
    dev = eng.to_device(masks)
    verts, loop_ptr, info, image_ptr, image_vert_ptr = (t.cpu().numpy() for t in eng.mask_outlines(dev, 8))
    assert image_ptr[0] == 0 and image_vert_ptr[0] == 0 and loop_ptr[0] == 0
    for b in range(3):
        one = [t.cpu().numpy() for t in eng.mask_outlines(dev[b:b + 1], 8)]
        lo, hi, vlo, vhi = image_ptr[b], image_ptr[b + 1], image_vert_ptr[b], image_vert_ptr[b + 1]
        assert one[3].tolist() == [0, hi - lo] and one[4].tolist() == [0, vhi - vlo] and hi > lo
        assert np.array_equal(one[0], verts[vlo:vhi]) and np.array_equal(one[2], info[lo:hi])
        assert np.array_equal(one[1], loop_ptr[lo:hi + 1] - vlo)
        assert int(info[lo:hi, 0].sum()) == int(masks[b].sum())         # the areas sum to the pixel count


# ---------------------------------------------------------------- the Python layer and the pipeline

def test_public_functions(eng):
    from gcn_grabcut import mask_outlines, mask_outlines_batch, outlines_to_lassos, polygon_mask
    m = np.pad(nested_rings(), 2) * 255
    for conn in (4, 8):
        got = mask_outlines(m, conn)
        want = ref.trace(m, conn)
        assert [(o.vertices.tolist(), o.area, o.perimeter, o.outer, o.hole) for o in got] == \
               [([list(v) for v in lp["vertices"]], lp["area"], lp["perimeter"], lp["outer"], lp["area"] < 0) for lp in want]
        assert all(o.vertices.dtype == np.int32 and o.vertices.shape[1] == 2 for o in got)
    both = mask_outlines_batch(np.stack([m, np.zeros_like(m)]).astype(bool))
    assert len(both) == 2 and both[1] == [] and len(both[0]) == 7
    solid = np.zeros((12, 14), np.uint8)
    solid[2:9, 3:11] = 1
    lasso, = outlines_to_lassos(mask_outlines(solid))
    # as a lasso the corner polygon covers its boundary too (H3): the pixels of the outline's bounding corners
    assert np.array_equal(polygon_mask(solid.shape, lasso)[2:9, 3:11], solid[2:9, 3:11])


@pytest.fixture(scope="module")
def pipe():
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig
    model, _ = seeded_state_dict(32, 2, seed=5)
    return GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=80), device="cuda")


def as_tuples(outlines):
    return [(o.vertices.tolist(), o.area, o.perimeter, o.outer) for o in outlines]


def test_result_outlines_and_no_new_kernel_in_a_plain_segment(pipe):
    from gcn_grabcut import mask_outlines
    from gcn_grabcut.synthetic import synthetic_image
    img = synthetic_image(90, 120, 30001)
    ctx = pipe._eng.ctx
    ctx.profile_enable(1)
    try:
        res = pipe.segment(img, min_area_ratio=0.0)
        assert [ctx.profile_query(n)[0] for n in SCOPES] == [0] * len(SCOPES)          # a plain segment launches none of them
        got = res.outlines()
        assert all(ctx.profile_query(n)[0] >= 1 for n in SCOPES)
    finally:
        ctx.profile_enable(0)
    assert res.binary_mask.any()
    assert as_tuples(got) == as_tuples(mask_outlines(res.binary_mask))
    assert as_tuples(got) == [([list(v) for v in lp["vertices"]], lp["area"], lp["perimeter"], lp["outer"])
                              for lp in ref.trace(res.binary_mask, 8)]
    assert as_tuples(res.outlines(4)) == as_tuples(mask_outlines(res.binary_mask, 4))
    with pytest.raises(ValueError, match="full"):
        res.outlines(full=True)
    big = synthetic_image(180, 240, 30001)
    res = pipe.segment(img, min_area_ratio=0.0, full_image=big)
    assert res.full is not None and res.full.binary_mask.shape == (180, 240)
    assert as_tuples(res.outlines(full=True)) == as_tuples(mask_outlines(res.full.binary_mask))
    assert as_tuples(res.outlines()) == as_tuples(mask_outlines(res.binary_mask))


def test_cli_writes_outlines_that_fill_back_to_the_saved_mask(tmp_path):
    from PIL import Image
    from gcn_grabcut.synthetic import synthetic_image
    img = synthetic_image(150, 200, 30003)
    Image.fromarray(img[:, :, ::-1]).save(tmp_path / "x.png")
    model, sd = seeded_state_dict(32, 2, seed=8)
    torch.save({"model": sd, "epoch": 1}, tmp_path / "ckpt.pt")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--image", str(tmp_path / "x.png"), "--output", str(out),
                        "--checkpoint", str(tmp_path / "ckpt.pt"), "--superpixels", "100", "--max-size", "100",
                        "--min-area", "0", "--save", "mask", "outlines", "--outline-connectivity", "4"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    mask = np.asarray(Image.open(out / "x_mask.png")) != 0
    doc = json.loads((out / "x_outlines.json").read_text())
    assert (doc["height"], doc["width"], doc["connectivity"]) == (75, 100, 4) == mask.shape + (4,)
    loops = [[tuple(v) for v in lp["vertices"]] for lp in doc["loops"]]
    assert np.array_equal(ref.fill_back(mask.shape, loops, polygons_ref.covered_np), mask)
    assert sum(lp["area"] for lp in doc["loops"]) == int(mask.sum())
    assert doc["svg_path"].count("M ") == doc["svg_path"].count(" Z") == len(loops)
    want = ref.trace(mask, 4)
    assert [(lp["area"], lp["perimeter"], lp["outer"]) for lp in doc["loops"]] == [(lp["area"], lp["perimeter"], lp["outer"]) for lp in want]
