"""Brush strokes on the MI355X: ggc_apply_strokes and ggc_stroke_pixels against the integer restatement of their rule
(tests/strokes_ref.py), then the pipeline with strokes (hard constraints, chunked runs, superpixel regions, the prior, the
geodesic mode), GrabCut.add_strokes + refine, and the CLI's stroke flags."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import strokes_ref
from helpers import seeded_state_dict

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
POISON = 7


@pytest.fixture(scope="module")
def eng():
    from gcn_grabcut._engine import get_engine
    return get_engine("cuda")


def _apply(eng, masks, per_image, radius):
    """ggc_apply_strokes through ctx.call on a (B,H,W) uint8 batch; per_image: a list of segments per image."""
    strokes, ptr = strokes_ref.pack(per_image)
    d_strokes, d_ptr = eng.upload_strokes(strokes, ptr)
    m = eng.to_device(np.ascontiguousarray(masks))
    b, h, w = m.shape
    eng.ctx.call("ggc_apply_strokes", eng._stream(), b, h, w, d_strokes.data_ptr() if len(strokes) else None,
                 d_ptr.data_ptr(), int(radius), m.data_ptr())
    return m.cpu().numpy()


def _pixels(eng, shape, per_image, fill=True, raw=False):
    """ggc_stroke_pixels through ctx.call: the count-only call, then (fill=True) the fill -> (hint_ptr, rows | None).
    raw=True checks nothing and returns what both calls wrote: (hint_ptr of the count-only call, rows, hint_ptr of the
    fill, the spare row), for a caller that reports differences itself."""
    strokes, ptr = strokes_ref.pack(per_image)
    d_strokes, d_ptr = eng.upload_strokes(strokes, ptr)
    b, h, w = shape
    hp = torch.full((b + 1,), -5, dtype=torch.int32, device=eng.device)
    args = (eng._stream(), b, h, w, d_strokes.data_ptr() if len(strokes) else None, d_ptr.data_ptr())
    eng.ctx.call("ggc_stroke_pixels", *args, hp.data_ptr(), None, 0)
    counted = hp.cpu().numpy()
    if not fill:
        return counted, None
    n = int(counted[-1])
    rows = torch.full((n + 1, 3), -9, dtype=torch.int32, device=eng.device)      # one spare row: it must stay untouched
    hp2 = torch.full((b + 1,), -5, dtype=torch.int32, device=eng.device)
    eng.ctx.call("ggc_stroke_pixels", *args, hp2.data_ptr(), rows.data_ptr(), n)
    if raw:
        rows = rows.cpu().numpy()
        return counted, rows[:n], hp2.cpu().numpy(), rows[n]
    assert np.array_equal(hp2.cpu().numpy(), counted)                   # the count-only call equals the fill call
    rows = rows.cpu().numpy()
    assert (rows[n] == -9).all()
    return counted, rows[:n]


def _base_batch(h=37, w=53):
    """B = 3, the middle image without strokes; mixed polylines, overlaps, endpoints outside the frame."""
    rng = np.random.default_rng(21)

    def polyline(n):
        return [(int(rng.integers(-15, h + 15)), int(rng.integers(-15, w + 15))) for _ in range(n)]
    img0 = strokes_ref.segments_of([polyline(4), [(5, 5)], polyline(2)], [polyline(3), [(-2, 10), (h + 3, 12)]])
    img2 = strokes_ref.segments_of([[(0, 0), (h - 1, w - 1)], [(h - 1, 0), (0, w - 1)]],       # the two diagonals ...
                                   [[(h // 2, -20), (h // 2, w + 20)], polyline(5), [(h - 1, w - 1)]])   # ... crossed
    return [img0, [], img2]


@pytest.mark.parametrize("radius", [0, 1, 5, 40])
def test_apply_strokes_matches_the_restatement(eng, radius):
    h, w = 37, 53
    per_image = _base_batch(h, w)
    rng = np.random.default_rng(radius)
    masks = rng.integers(0, 4, (3, h, w)).astype(np.uint8)
    got = _apply(eng, masks, per_image, radius)
    for b in range(3):
        assert np.array_equal(got[b], strokes_ref.paint(masks[b], per_image[b], radius)), (b, radius)
    assert np.array_equal(got[1], masks[1])
    for b in range(3):                                                  # every image equals its single-image call
        assert np.array_equal(_apply(eng, masks[b:b + 1], [per_image[b]], radius)[0], got[b]), (b, radius)
    # pixels no stroke touches are not written: they keep a poison value
    got = _apply(eng, np.full((3, h, w), POISON, np.uint8), per_image, radius)
    for b in range(3):
        lab = strokes_ref.labels(h, w, per_image[b], radius)
        assert np.array_equal(got[b] == POISON, lab < 0), (b, radius)


def test_apply_strokes_more_segments_than_one_culling_pass(eng):
    """300 short segments on one image: the culled list takes a second pass, and the last segment wins across it."""
    rng = np.random.default_rng(5)
    h, w = 45, 70
    segs = []
    for k in range(300):
        r, c = int(rng.integers(0, 14)), int(rng.integers(0, 24))       # all inside one corner: its tiles keep them all
        segs.append((r, c, r + int(rng.integers(-3, 4)), c + int(rng.integers(-3, 4)), int(rng.integers(0, 2))))
    segs[10] = (6, 3, 6, 20, 1)                                         # first pass ...
    segs[290] = (3, 12, 10, 12, 0)                                      # ... crossed by one of the second pass
    masks = np.full((2, h, w), POISON, np.uint8)
    got = _apply(eng, masks, [segs, [(20, 30, 20, 30, 1)]], 2)
    assert np.array_equal(got[0], strokes_ref.paint(masks[0], segs, 2))
    assert np.array_equal(got[1], strokes_ref.paint(masks[1], [(20, 30, 20, 30, 1)], 2))
    late = strokes_ref.labels(h, w, segs[256:], 2)
    assert (late >= 0).any() and np.array_equal(got[0][late >= 0], late[late >= 0])


def test_apply_strokes_exact_tangency(eng):
    cases = [((5, 5, 17, 21, 1), 5),                                    # direction 3-4-5
             ((10, 4, 10, 30, 1), 5), ((4, 10, 30, 10, 0), 5),          # axis-aligned
             ((5, 5, 25, 25, 1), 5), ((25, 5, 5, 25, 0), 5),            # 45 degrees
             ((5, 5, 25, 25, 1), 0), ((5, 5, 6, 25, 1), 0), ((5, 5, 25, 6, 0), 0), ((3, 3, 4, 4, 1), 0),
             ((2, 2, 2, 2, 1), 0), ((2, 2, 2, 2, 1), 1)]
    masks = np.full((1, 40, 40), POISON, np.uint8)
    for seg, radius in cases:
        got = _apply(eng, masks, [[seg]], radius)[0]
        assert np.array_equal(got, strokes_ref.paint(masks[0], [seg], radius)), (seg, radius)
    got = _apply(eng, masks, [[cases[0][0]]], 5)[0]
    assert got[15, 10] == 1 and got[16, 10] == POISON                   # exactly at distance 5 / just beyond
    # radius 0, pixels beside the line: (0,0)->(1,2) passes between (0,1) and (1,1), the diagonal keeps clear of its neighbours
    got = _apply(eng, masks, [[(0, 0, 1, 2, 1)]], 0)[0]
    assert got[0, 1] == 1 and got[1, 1] == 1                            # both at distance 1/sqrt(5) < 1/2
    got = _apply(eng, masks, [[(0, 0, 2, 2, 1)]], 0)[0]
    assert got[0, 1] == POISON and got[1, 0] == POISON                  # sqrt(1/2) > 1/2
    got = _apply(eng, masks, [[(0, 0, 1, 1, 1), (1, 0, 0, 1, 1)]], 0)[0]
    assert (got[:2, :2] == 1).all()


def test_apply_strokes_long_segments_need_128_bits(eng):
    for i, ((h, w), seg, radius) in enumerate(strokes_ref.LONG_CASES):
        masks = np.full((1, h, w), POISON, np.uint8)
        got = _apply(eng, masks, [[seg]], radius)[0]
        assert np.array_equal(got, strokes_ref.paint(masks[0], [seg], radius)), i
        assert (got != POISON).any(), i


@pytest.mark.parametrize("radius", [0, 3, 6])
def test_one_vertex_stroke_equals_apply_hints(eng, radius):
    h, w = 37, 53
    pts = [(0, 0, 1), (h - 1, w - 1, 0), (18, 30, 1), (19, 33, 0), (36, 2, 1)]
    a = torch.full((1, h, w), POISON, dtype=torch.uint8, device=eng.device)
    b = a.clone()
    d_strokes, d_ptr = eng.upload_strokes(np.asarray([(r, c, r, c, l) for r, c, l in pts], np.int32), np.array([0, len(pts)]))
    eng.apply_strokes(a, d_strokes, d_ptr, radius)
    hints, hint_ptr = eng.upload_hints(np.asarray(pts, np.int32), np.array([0, len(pts)]))
    eng.apply_hints(b, hints, hint_ptr, radius)
    assert torch.equal(a, b) and bool((a != POISON).any())


def test_stroke_pixels_matches_the_restatement(eng):
    h, w = 37, 53
    per_image = _base_batch(h, w)
    ptr, rows = _pixels(eng, (3, h, w), per_image)
    want = [strokes_ref.pixels(h, w, segs) for segs in per_image]
    assert ptr.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in want])]).tolist()
    assert ptr[1] == ptr[2]                                             # the image without strokes
    assert np.array_equal(rows, np.concatenate(want))                   # the same set, raster order, the same labels
    assert len(want[0]) and len(want[2]) and {0, 1} <= set(rows[:, 2].tolist())
    # the last image alone without strokes; a wide image whose rows span several 64-lane steps
    ptr, rows = _pixels(eng, (2, 5, 300), [[(2, -4, 3, 310, 1), (0, 150, 4, 150, 0)], []])
    want = strokes_ref.pixels(5, 300, [(2, -4, 3, 310, 1), (0, 150, 4, 150, 0)])
    assert ptr.tolist() == [0, len(want), len(want)] and np.array_equal(rows, want)


def test_stroke_pixels_capacity_and_no_ops(eng):
    from gcn_grabcut import _native
    h, w = 20, 30
    segs = [(2, 2, 15, 25, 1)]
    strokes, ptr = strokes_ref.pack([segs])
    d_strokes, d_ptr = eng.upload_strokes(strokes, ptr)
    n = len(strokes_ref.pixels(h, w, segs))
    hp = torch.zeros(2, dtype=torch.int32, device=eng.device)
    rows = torch.full((n, 3), -9, dtype=torch.int32, device=eng.device)
    with pytest.raises(_native.GGCError, match="INVALID_ARG"):          # one row too few: refused, nothing written
        eng.ctx.call("ggc_stroke_pixels", eng._stream(), 1, h, w, d_strokes.data_ptr(), d_ptr.data_ptr(), hp.data_ptr(),
                     rows.data_ptr(), n - 1)
    assert bool((rows == -9).all()) and hp.tolist() == [0, n]
    # no segments: hint_ptr_out is all zeros, hints_out untouched; B == 0 writes nothing at all
    _, empty = eng.upload_strokes(np.zeros((0, 5), np.int32), np.zeros(3, np.int32))
    hp = torch.full((3,), -5, dtype=torch.int32, device=eng.device)
    eng.ctx.call("ggc_stroke_pixels", eng._stream(), 2, h, w, None, empty.data_ptr(), hp.data_ptr(), rows.data_ptr(), n)
    assert hp.tolist() == [0, 0, 0] and bool((rows == -9).all())
    hp.fill_(-5)
    eng.ctx.call("ggc_stroke_pixels", eng._stream(), 0, h, w, None, None, hp.data_ptr(), None, 0)
    assert hp.tolist() == [-5, -5, -5]
    # strokes that miss the image entirely: zero pixels, and the fill call with capacity 0 is fine
    ptr_out, rows_out = _pixels(eng, (1, h, w), [[(-50, -50, -40, 200, 1)]])
    assert ptr_out.tolist() == [0, 0] and rows_out.shape == (0, 3)
    mask = torch.full((2, h, w), POISON, dtype=torch.uint8, device=eng.device)
    eng.ctx.call("ggc_apply_strokes", eng._stream(), 2, h, w, None, empty.data_ptr(), 3, mask.data_ptr())
    eng.ctx.call("ggc_apply_strokes", eng._stream(), 0, h, w, None, None, 3, None)
    assert bool((mask == POISON).all())


def test_stroke_argument_checks(eng):
    from gcn_grabcut import _native
    h, w = 9, 11
    mask = torch.full((2, h, w), POISON, dtype=torch.uint8, device=eng.device)
    hp = torch.full((3,), -5, dtype=torch.int32, device=eng.device)
    rows = torch.full((4, 3), -9, dtype=torch.int32, device=eng.device)
    one = np.array([[1, 1, 5, 5, 1]], np.int32)
    good, ptr = eng.upload_strokes(one, np.array([0, 1, 1], np.int32))
    st = eng._stream()

    def refused(name, code, *args):
        with pytest.raises(_native.GGCError, match=code) as e:
            eng.ctx.call(name, st, *args)
        assert str(e.value).split(": ", 1)[1].strip(), name             # with a message from ggc_last_error

    def both(code, strokes, stroke_ptr, b=2, hh=h, ww=w):
        refused("ggc_apply_strokes", code, b, hh, ww, _native.ptr(strokes), _native.ptr(stroke_ptr), 2, mask.data_ptr())
        refused("ggc_stroke_pixels", code, b, hh, ww, _native.ptr(strokes), _native.ptr(stroke_ptr), hp.data_ptr(), None, 0)

    for bad in ([1, 1, 1], [0, 2, 1]):                                  # not starting at 0; decreasing
        both("INVALID_ARG", *eng.upload_strokes(np.repeat(one, 2, 0), np.array(bad, np.int32)))
    for j, v in ((0, 2**20 + 1), (1, -2**20 - 1), (2, 2**21), (3, -2**30)):   # an endpoint beyond +-2^20
        row = one.copy()
        row[0, j] = v
        both("INVALID_ARG", *eng.upload_strokes(row, np.array([0, 1, 1], np.int32)))
    both("INVALID_ARG", None, ptr)                                      # NULL strokes with a segment
    both("INVALID_ARG", good, None)                                     # NULL stroke_ptr
    both("SHAPE", good, ptr, hh=0)
    both("SHAPE", good, ptr, ww=65536)
    both("SHAPE", good, ptr, b=65536)
    for radius in (-1, 16385):
        refused("ggc_apply_strokes", "INVALID_ARG", 2, h, w, good.data_ptr(), ptr.data_ptr(), radius, mask.data_ptr())
    refused("ggc_apply_strokes", "INVALID_ARG", 2, h, w, good.data_ptr(), ptr.data_ptr(), 2, None)          # NULL mask
    refused("ggc_stroke_pixels", "INVALID_ARG", 2, h, w, good.data_ptr(), ptr.data_ptr(), None, None, 0)    # NULL hint_ptr_out
    refused("ggc_stroke_pixels", "INVALID_ARG", 2, h, w, good.data_ptr(), ptr.data_ptr(), hp.data_ptr(), rows.data_ptr(), -1)
    assert bool((mask == POISON).all()) and hp.tolist() == [-5, -5, -5] and bool((rows == -9).all())   # refused before any launch
    ok, okp = eng.upload_strokes(np.array([[2**20, -2**20, -2**20, 2**20, 1]], np.int32), np.array([0, 1, 1], np.int32))
    eng.ctx.call("ggc_apply_strokes", st, 2, h, w, ok.data_ptr(), okp.data_ptr(), 16384, mask.data_ptr())   # the limits themselves
    assert bool((mask[0] == 1).all()) and bool((mask[1] == POISON).all())


def test_public_paint_strokes_and_stroke_pixels():
    from gcn_grabcut import paint_strokes, stroke_pixels
    fg, bg = [[(2, 2), (20, 40), (30, 10)]], [[(0, 30), (36, 30)], [(10, 10)]]
    segs = strokes_ref.segments_of(fg, bg)
    m = np.random.default_rng(2).integers(0, 4, (37, 53)).astype(np.uint8)
    assert np.array_equal(paint_strokes(m, fg, bg, 4), strokes_ref.paint(m, segs, 4))
    assert np.array_equal(paint_strokes((37, 53), fg, bg), strokes_ref.paint(np.full((37, 53), 2, np.uint8), segs, 3))
    assert np.array_equal(stroke_pixels((37, 53), fg, bg), strokes_ref.pixels(37, 53, segs))
    assert stroke_pixels((37, 53), [], []).shape == (0, 3)


# ---------------------------------------------------------------- pipeline

H, W = 96, 128
STROKED = (0, 2)
RADIUS = 4
KEYS = ("binary_mask", "trimap", "segments", "probs", "gc_mask", "overlay", "rgba")


def _batch_strokes():
    return [([], [[(H // 2, -10), (H // 2 + 6, W + 10)]]),                                   # background across the object
            None,
            ([[(20, 20), (H // 2, W // 2), (H - 15, W // 2 + 30)], [(10, W - 10)]], [[(H - 5, 5), (H - 5, 40)]]),
            None]


@pytest.fixture(scope="module")
def stroked_runs():
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig
    from gcn_grabcut.synthetic import synthetic_batch
    model, sd = seeded_state_dict(32, 2, seed=5)
    pipe = GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=80), device="cuda")
    imgs = synthetic_batch(4, H, W, config_id=9)
    bgr = pipe._eng.to_device(imgs)
    strokes = _batch_strokes()
    kw = dict(chunks=1, min_area_ratio=0.0, return_state=True)
    base = pipe.segment_batch_device(bgr, **kw)
    stroked = pipe.segment_batch_device(bgr, strokes=strokes, stroke_radius=RADIUS, **kw)
    return pipe, imgs, bgr, strokes, base, stroked


def _segs(strokes, b):
    return strokes_ref.segments_of(*strokes[b])


def test_pipeline_strokes_are_hard_constraints(stroked_runs):
    pipe, imgs, bgr, strokes, base, stroked = stroked_runs
    seen = set()
    for b in STROKED:
        lab = strokes_ref.labels(H, W, _segs(strokes, b), RADIUS)
        tri = stroked["trimap"][b].cpu().numpy()
        assert np.array_equal(tri, strokes_ref.paint(base["trimap"][b].cpu().numpy(), _segs(strokes, b), RADIUS)), b
        gc_mask, gc_bin = stroked["gc_mask"][b].cpu().numpy(), stroked["gc_binary"][b].cpu().numpy()
        binm = stroked["binary_mask"][b].cpu().numpy()
        for l in (0, 1):
            if (lab == l).any():
                seen.add(l)
                assert (gc_mask[lab == l] == l).all(), (b, l)            # GC_BGD / GC_FGD on every brush pixel
                assert (gc_bin[lab == l] == l).all(), (b, l)
                assert (binm[lab == l] == l).all(), (b, l)               # (no clean-up in these runs)
    assert seen == {0, 1}
    lab0 = strokes_ref.labels(H, W, _segs(strokes, 0), RADIUS)
    assert (base["gc_binary"][0].cpu().numpy()[lab0 == 0] == 1).any()   # the background stroke did cross the object


def test_pipeline_strokes_leave_other_images_alone(stroked_runs):
    pipe, imgs, bgr, strokes, base, stroked = stroked_runs
    g0 = base["graphs"]
    for b in range(4):
        if b in STROKED:
            continue
        for k in ("binary_mask", "trimap", "segments", "gc_mask", "gc_binary", "overlay", "rgba", "bgd", "fgd"):
            assert torch.equal(base[k][b], stroked[k][b]), (b, k)
    assert torch.equal(base["probs"], stroked["probs"])                 # hard constraints do not touch the network
    assert torch.equal(g0.x, stroked["graphs"].x)


def test_pipeline_strokes_chunked_equals_one_chunk(stroked_runs):
    pipe, imgs, bgr, strokes, base, stroked = stroked_runs
    clicks = [None, ([(5, 5)], []), ([(H - 3, W - 3)], [(30, 30)]), None]
    for kw in (dict(), dict(hints=clicks, hint_radius=3, hint_region=True, hints_as_prior=True)):
        one = stroked if not kw else pipe.segment_batch_device(bgr, chunks=1, min_area_ratio=0.0, strokes=strokes,
                                                               stroke_radius=RADIUS, **kw)
        two = pipe.segment_batch_device(bgr, chunks=2, min_area_ratio=0.0, strokes=strokes, stroke_radius=RADIUS, **kw)
        for k in KEYS:
            assert torch.equal(one[k], two[k]), (k, bool(kw))
        assert not torch.equal(one["trimap"], base["trimap"])


def test_pipeline_without_strokes_is_the_call_without_the_argument(stroked_runs):
    pipe, imgs, bgr, strokes, base, stroked = stroked_runs
    from gcn_grabcut.graph_builder import pack_strokes
    for arg in (None, [None] * 4, [None, ([], []), None, ((), None)]):
        out = pipe.segment_batch_device(bgr, chunks=1, min_area_ratio=0.0, strokes=arg)
        for k in KEYS:
            assert torch.equal(out[k], base[k]), k
    segs, ptr = pack_strokes(strokes)                                   # the packed pair equals the per-image lists
    out = pipe.segment_batch_device(bgr, chunks=1, min_area_ratio=0.0, strokes=(torch.from_numpy(segs), torch.from_numpy(ptr)),
                                    stroke_radius=RADIUS)
    for k in KEYS:
        assert torch.equal(out[k], stroked[k]), k
    res = pipe.segment_batch(list(imgs), strokes=strokes, stroke_radius=RADIUS, min_area_ratio=0.0, chunks=1)
    for b in range(4):
        assert np.array_equal(res[b].binary_mask, stroked["binary_mask"][b].cpu().numpy()), b
    fg, bg = strokes[2]
    r = pipe.segment(imgs[2], fg_strokes=fg, bg_strokes=bg, stroke_radius=RADIUS, min_area_ratio=0.0)
    one = pipe.segment_batch_device(bgr[2:3], strokes=[strokes[2]], stroke_radius=RADIUS, min_area_ratio=0.0)
    assert np.array_equal(r.trimap, one["trimap"][0].cpu().numpy())
    assert np.array_equal(r.binary_mask, one["binary_mask"][0].cpu().numpy())


def test_pipeline_stroke_region_and_prior(stroked_runs):
    from gcn_grabcut.graph_builder import encode_user_hints
    pipe, imgs, bgr, strokes, base, stroked = stroked_runs
    clicks = [None, None, ([], [(20, 20), (5, 100)]), ([(40, 40)], [])]  # (20,20): a background click on a foreground stroke's vertex
    seg = base["segments"].cpu().numpy()
    merged = {}
    for b in range(4):
        pix = strokes_ref.pixels(H, W, _segs(strokes, b)) if strokes[b] is not None else np.zeros((0, 3), np.int32)
        fg, bg = clicks[b] if clicks[b] is not None else ([], [])
        merged[b] = [tuple(int(v) for v in p) for p in pix] + [(r, c, 1) for r, c in fg] + [(r, c, 0) for r, c in bg]
    # hint_region: radius-0 brush and clicks, so that nothing but the centre lines, the clicks and the regions is painted
    out = pipe.segment_batch_device(bgr, chunks=1, strokes=strokes, stroke_radius=0, hints=clicks, hint_radius=0, hint_region=True)
    assert torch.equal(out["probs"], base["probs"])
    for b in range(4):
        want = base["trimap"][b].cpu().numpy().copy()
        by_region = {}
        for r, c, l in merged[b]:
            by_region.setdefault(int(seg[b][r, c]), set()).add(l)
        definite = 0
        for s, ls in by_region.items():
            if len(ls) == 1:                                            # crossed by one label only: the whole superpixel
                want[seg[b] == s] = ls.pop()
                definite += 1
        if strokes[b] is not None:
            want = strokes_ref.paint(want, _segs(strokes, b), 0)
        for l, pts in ((1, clicks[b][0]), (0, clicks[b][1])) if clicks[b] is not None else ():
            for r, c in pts:                                            # the clicks, after the strokes
                want[r, c] = l
        assert np.array_equal(out["trimap"][b].cpu().numpy(), want), b
        assert definite >= (3 if b in STROKED else 0), b
    # hints_as_prior: x[:, 16:19] of exactly the nodes under a centre line or a click
    out = pipe.segment_batch_device(bgr, chunks=1, strokes=strokes, stroke_radius=RADIUS, hints=clicks, hint_radius=3,
                                    hints_as_prior=True)
    g = base["graphs"]
    x = g.x.clone()
    for b in range(4):
        if not merged[b]:
            continue
        n0, n1 = g.node_ptr_host[b], g.node_ptr_host[b + 1]
        table = encode_user_hints(seg[b], [(r, c) for r, c, l in merged[b] if l == 1], [(r, c) for r, c, l in merged[b] if l == 0])
        assert (table[:, :2].sum(1) > 0).any()
        x[n0:n1, 16:19] = torch.from_numpy(table).to(x.device)
    assert torch.equal(out["graphs"].x, x)
    n0, n1 = g.node_ptr_host[1], g.node_ptr_host[2]                     # image 1 has neither: the automatic prior
    assert torch.equal(out["graphs"].x[n0:n1], g.x[n0:n1]) and torch.equal(out["probs"][n0:n1], base["probs"][n0:n1])


def test_pipeline_strokes_in_geodesic_mode(stroked_runs):
    from gcn_grabcut import geodesic_hints
    pipe, imgs, bgr, strokes, base, stroked = stroked_runs
    clicks = [None, None, ([(H - 3, W - 3)], []), None]
    out = pipe.segment_batch_device(bgr, chunks=1, strokes=strokes, stroke_radius=RADIUS, hints=clicks, geodesic=True)
    for b in range(4):
        tri0 = base["trimap"][b].cpu().numpy()
        if b not in STROKED:
            assert np.array_equal(out["trimap"][b].cpu().numpy(), tri0), b
            continue
        pix = strokes_ref.pixels(H, W, _segs(strokes, b))
        fg = [(r, c) for r, c, l in pix if l == 1] + (clicks[b][0] if clicks[b] else [])
        bg = [(r, c) for r, c, l in pix if l == 0] + (clicks[b][1] if clicks[b] else [])
        want = geodesic_hints(imgs[b], fg, bg, mask=tri0)
        assert np.array_equal(out["trimap"][b].cpu().numpy(), want), b
        assert not np.array_equal(want, tri0), b


# ---------------------------------------------------------------- GrabCut.add_strokes

def test_grabcut_add_strokes_then_refine():
    from gcn_grabcut import GrabCut
    from gcn_grabcut.synthetic import synthetic_image
    img = synthetic_image(70, 90, 1234)
    gc = GrabCut(img, device="cuda")
    with pytest.raises(RuntimeError):
        gc.add_strokes(fg_strokes=[[(5, 5)]])
    tri = np.full((70, 90), 2, np.uint8)
    tri[20:50, 25:65] = 3
    tri[30:40, 35:55] = 1
    tri[:4] = 0
    gc.run_with_trimap(tri)
    m0 = gc.mask.copy()
    fg, bg = [[(60, 5), (64, 30)], [(8, 80)]], [[(25, 30), (45, 60), (45, 30)]]
    gc.add_strokes(fg_strokes=fg, bg_strokes=bg, radius=3)
    segs = strokes_ref.segments_of(fg, bg)
    assert np.array_equal(gc.mask, strokes_ref.paint(m0, segs, 3))
    assert gc.history[-1].tag == "strokes"
    binary = gc.refine(1)
    lab = strokes_ref.labels(70, 90, segs, 3)
    assert (lab == 1).any() and (lab == 0).any()
    assert (gc.mask[lab == 1] == 1).all() and (gc.mask[lab == 0] == 0).all()        # refine keeps the brush pixels
    assert (binary[lab == 1] == 1).all() and (binary[lab == 0] == 0).all()


# ---------------------------------------------------------------- CLI

def test_cli_takes_a_background_stroke(tmp_path):
    from PIL import Image
    from gcn_grabcut.synthetic import synthetic_image
    img = synthetic_image(300, 400, 4242)
    Image.fromarray(img[:, :, ::-1]).save(tmp_path / "x.png")
    model, sd = seeded_state_dict(32, 2, seed=8)
    torch.save({"model": sd, "epoch": 1}, tmp_path / "ckpt.pt")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--image", str(tmp_path / "x.png"), "--output", str(out),
                        "--checkpoint", str(tmp_path / "ckpt.pt"), "--superpixels", "100", "--max-size", "200",
                        "--min-area", "0", "--save", "mask", "--bg-stroke", "150,-20 150,200 290,390", "--fg-stroke", "20,20",
                        "--stroke-radius", "2"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    mask = np.asarray(Image.open(out / "x_mask.png"))
    assert mask.shape == (150, 200)                                     # the --max-size resize halved the image
    lab = strokes_ref.labels(150, 200, strokes_ref.segments_of([[(10, 10)]], [[(75, -10), (75, 100), (145, 195)]]), 2)
    assert (lab == 0).sum() > 200
    assert (mask[lab == 1] == 255).all() and (mask[lab == 0] == 0).all()
