"""Intelligent scissors on the MI355X: ggc_trace_paths against the integer restatement of its definition
(tests/scissors_ref.py), vertex for vertex and distance for distance, then the painter fed with a traced batch, the
pipeline with scissors, segment_scissors and the CLI's --scissors."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import geodesic_ref
import polygons_ref
import scissors_ref as ref
from helpers import seeded_state_dict

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
POISON = -7
DEFAULTS = (16, 2048, 16)
SETTINGS = [(0, 2048, 16), (16, 2048, 16), (5, 1, 1), (256, 13770, 64), (16, 512, 64)]


@pytest.fixture(scope="module")
def eng():
    from gcn_grabcut._engine import get_engine
    return get_engine("cuda")


def _trace(eng, images, paths, setting):
    """paths: per image None or [(anchors, closed)] -> (verts, vert_ptr) on the host, through Engine.trace_paths."""
    from gcn_grabcut.graph_builder import pack_paths
    packed = pack_paths([None if not p else [(a, bool(c)) for a, c in p] for p in paths])
    bgr = eng.to_device(np.ascontiguousarray(np.stack(images)))
    verts, vert_ptr = eng.trace_paths(bgr, *eng.upload_paths(*packed), *setting)
    return verts.cpu().numpy(), vert_ptr.cpu().numpy()


H0, W0 = 37, 53      # no multiple of the 32x32 tile


def _kernel_images():
    from gcn_grabcut.synthetic import synthetic_image
    rng = np.random.default_rng(11)
    imgs = [synthetic_image(H0, W0, 500 + i) for i in range(6)]
    imgs[3] = rng.integers(0, 256, (H0, W0, 3)).astype(np.uint8)                       # noise: hardly a tie
    imgs[4] = (imgs[4].astype(np.int32) + rng.integers(-20, 21, (H0, W0, 3))).clip(0, 255).astype(np.uint8)
    return imgs


def _kernel_paths():
    """Image 1 has no path.  Open and closed paths of 2..7 anchors; anchors on the border and in the corners; consecutive
    equal anchors; segments inside one tile ((2,2)->(10,20)) and across the corner where four tiles meet ((30,30)->(33,34))."""
    return [
        [([(0, 0), (0, 52), (36, 52)], True), ([(5, 5), (30, 45)], False)],
        None,
        [([(2, 2), (10, 20), (10, 20), (30, 30), (33, 34), (33, 34), (12, 50)], False), ([(31, 31), (32, 32)], False)],
        [([(0, 10), (18, 52), (36, 30), (20, 0)], True), ([(4, 4), (4, 40), (30, 44), (33, 8), (18, 2)], True)],
        [([(36, 0), (20, 20), (8, 31), (8, 32), (25, 52), (0, 52)], False), ([(3, 3), (3, 3), (9, 9)], True)],
        [([(1, 26), (10, 45), (28, 48), (35, 26), (28, 5), (10, 3), (5, 15)], True), ([(36, 0), (36, 0)], False)],
    ]


@pytest.fixture(scope="module")
def kernel_batch():
    return _kernel_images(), _kernel_paths()


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "m%d-e%d-s%d" % s)
def test_kernel_batch_matches_the_reference(eng, kernel_batch, setting):
    imgs, paths = kernel_batch
    want_v, want_p = ref.trace_batch(imgs, paths, *setting)
    got_v, got_p = _trace(eng, imgs, paths, setting)
    assert np.array_equal(got_p, want_p)
    assert np.array_equal(got_v, want_v)
    assert got_p[-1] - got_p[-2] == 1 and tuple(got_v[-1]) == (36, 0)      # the open path of two equal anchors: one vertex


def test_distance_planes_match_the_reference(eng, kernel_batch):
    imgs, paths = kernel_batch
    planes = []
    want_v, _ = ref.trace_batch(imgs, paths, *DEFAULTS, planes=planes)
    got_v, _ = _trace(eng, imgs, paths, DEFAULTS)
    want = np.concatenate(planes).astype(np.int32)
    got = np.empty_like(want)
    eng.ctx.call("ggc_debug_read_scratch", b"scissors_planes", got.ctypes.data, got.nbytes)
    assert np.array_equal(got, want)
    assert np.array_equal(got_v, want_v)


def test_batch_equals_single_path_calls_and_repeats(eng, kernel_batch):
    imgs, paths = kernel_batch
    got_v, got_p = _trace(eng, imgs, paths, DEFAULTS)
    again = _trace(eng, imgs, paths, DEFAULTS)
    assert np.array_equal(again[0], got_v) and np.array_equal(again[1], got_p)
    q = 0
    for img, ps in zip(imgs, paths):
        for p in ps or []:
            one_v, one_p = _trace(eng, [img], [[p]], DEFAULTS)
            assert np.array_equal(one_p, [0, got_p[q + 1] - got_p[q]]), q
            assert np.array_equal(one_v, got_v[got_p[q]:got_p[q + 1]]), q
            q += 1
    assert q == len(got_p) - 1


@pytest.mark.parametrize("shape", [(64, 64), (33, 65)], ids=lambda s: "%dx%d" % s)
def test_constant_images_follow_the_tie_rule(eng, shape):
    h, w = shape
    img = np.full((h, w, 3), 90, np.uint8)
    paths = [[([(0, 0), (h - 1, w - 1)], False), ([(h - 1, 0), (0, w - 1), (h // 2, w // 2)], True),
              ([(0, w - 1), (h - 1, 0)], False), ([(h - 1, w - 1), (0, 0), (0, w - 1), (h - 1, 2)], False)]]
    for setting in ((0, 2048, 16), (16, 2048, 16)):
        want_v, want_p = ref.trace_batch([img], paths, *setting)
        got_v, got_p = _trace(eng, [img], paths, setting)
        assert np.array_equal(got_p, want_p) and np.array_equal(got_v, want_v), setting


def test_many_rounds_on_a_walled_scene(eng):
    """geodesic_ref.serpentine: the only cheap crossings of a wall's flat middle row are at the wall's open end, alternately
    right and left, so with smooth 1 the cheapest path winds through the tiles again and again."""
    img = geodesic_ref.serpentine(70, 70)
    setting = (0, 2048, 1)
    path = [([(0, 0), (69, 69)], False)]
    want_v, want_p = ref.trace_batch([img], [path], *setting)
    assert len(want_v) > 4 * 70                                         # it does wind
    got_v, got_p = _trace(eng, [img], [path], setting)
    assert np.array_equal(got_p, want_p) and np.array_equal(got_v, want_v)
    other = _kernel_images()
    big = [np.ascontiguousarray(np.pad(o, ((0, 70 - H0), (0, 70 - W0), (0, 0)), mode="edge")) for o in other[:2]]
    paths3 = [[([(3, 3), (60, 60), (10, 66)], True)], [([(69, 0), (0, 69)], False)], path]
    want3 = ref.trace_batch([big[0], big[1], img], paths3, *setting)
    got3 = _trace(eng, [big[0], big[1], img], paths3, setting)
    assert np.array_equal(got3[1], want3[1]) and np.array_equal(got3[0], want3[0])
    assert np.array_equal(got3[0][got3[1][2]:], got_v)


def test_small_shapes(eng):
    rng = np.random.default_rng(3)
    one = rng.integers(0, 256, (1, 1, 3)).astype(np.uint8)
    v, p = _trace(eng, [one], [[([(0, 0), (0, 0)], False)]], DEFAULTS)
    assert np.array_equal(p, [0, 1]) and np.array_equal(v, [[0, 0]])
    row, col = rng.integers(0, 256, (1, 70, 3)).astype(np.uint8), rng.integers(0, 256, (70, 1, 3)).astype(np.uint8)
    for img, far in ((row, (0, 69)), (col, (69, 0))):
        mid = (far[0] // 2, far[1] // 2)
        paths = [[([(0, 0), far], False), ([far, mid, (0, 0)], True), ([mid, mid, far], False)]]
        for setting in (DEFAULTS, (0, 1, 1)):
            want = ref.trace_batch([img], paths, *setting)
            got = _trace(eng, [img], paths, setting)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
        assert got[1][1] == 70                                          # a line image: every pixel once, the anchor appended


@pytest.fixture(scope="module")
def large_scene():
    from gcn_grabcut.synthetic import synthetic_image
    img, gt = synthetic_image(300, 400, 30001, return_mask=True)
    _, anchors = ref.boundary_anchors(gt, 8)
    return img, anchors


def test_larger_scene_with_windows_of_several_tiles(eng, large_scene):
    img, anchors = large_scene
    spans = [max(abs(a[0] - b[0]), abs(a[1] - b[1])) for a, b in ref.segments(anchors, True)]
    assert max(spans) > 64                                              # windows of several tiles
    want = ref.trace_batch([img], [[(anchors, True)]], *DEFAULTS)
    got = _trace(eng, [img], [[(anchors, True)]], DEFAULTS)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


# ---------------------------------------------------------------- call behaviour

def _raw(eng, bgr, packed, setting=DEFAULTS, verts=None, capacity=0, vert_ptr=None, **over):
    from gcn_grabcut import _native
    b, h, w, _ = bgr.shape
    a, pp, pc, ip = packed
    args = dict(b=b, h=h, w=w, img=bgr, a=a, pp=pp, pc=pc, ip=ip, q=int(pc.numel()), margin=setting[0], edge_cap=setting[1],
                smooth=setting[2], vp=vert_ptr, verts=verts, capacity=capacity)
    args.update(over)
    P = _native.ptr
    return eng.ctx.call("ggc_trace_paths", eng._stream(), args["b"], args["h"], args["w"], P(args["img"]), P(args["a"]),
                        P(args["pp"]), P(args["pc"]), P(args["ip"]), args["q"], args["margin"], args["edge_cap"], args["smooth"],
                        P(args["vp"]), P(args["verts"]), args["capacity"])


def _count_then_fill(eng, bgr, packed, setting=DEFAULTS):
    """The two-call pattern on device arrays: count only, then the fill with exactly enough rows and one spare
    -> (vert_ptr of the count-only call, vert_ptr of the fill, verts (V,2), the spare row), on the host, unchecked."""
    q = int(packed[2].numel())
    vp = torch.full((q + 1,), POISON, dtype=torch.int32, device=eng.device)
    _raw(eng, bgr, packed, setting, vert_ptr=vp)
    count_ptr = vp.cpu().numpy()
    n = int(count_ptr[-1])
    verts = torch.full((n + 1, 2), POISON, dtype=torch.int32, device=eng.device)
    vp.fill_(POISON)
    _raw(eng, bgr, packed, setting, vert_ptr=vp, verts=verts, capacity=n)
    host = verts.cpu().numpy()
    return count_ptr, vp.cpu().numpy(), host[:n], host[n]


def test_count_only_capacity_and_no_ops(eng, kernel_batch):
    from gcn_grabcut import _native
    from gcn_grabcut.graph_builder import pack_paths
    imgs, paths = kernel_batch
    want_v, want_p = ref.trace_batch(imgs, paths, *DEFAULTS)
    bgr = eng.to_device(np.stack(imgs))
    packed = eng.upload_paths(*pack_paths([None if not p else [(a, bool(c)) for a, c in p] for p in paths]))
    q, n = len(want_p) - 1, len(want_v)
    vp = torch.full((q + 1,), POISON, dtype=torch.int32, device=eng.device)
    _raw(eng, bgr, packed, vert_ptr=vp)                                 # count only
    assert np.array_equal(vp.cpu().numpy(), want_p)
    verts = torch.full((n + 5, 2), POISON, dtype=torch.int32, device=eng.device)
    vp.fill_(POISON)
    with pytest.raises(_native.GGCError, match="INVALID_ARG"):          # capacity too small: verts_out untouched
        _raw(eng, bgr, packed, vert_ptr=vp, verts=verts, capacity=n - 1)
    assert bool((verts == POISON).all())
    assert np.array_equal(vp.cpu().numpy(), want_p)                     # vert_ptr_out is written all the same
    _raw(eng, bgr, packed, vert_ptr=vp, verts=verts, capacity=n)        # exactly enough
    got = verts.cpu().numpy()
    assert np.array_equal(got[:n], want_v) and (got[n:] == POISON).all()
    # the no-ops write nothing and look at nothing
    vp.fill_(POISON)
    verts.fill_(POISON)
    _raw(eng, bgr, packed, vert_ptr=vp, verts=verts, capacity=n, b=0)
    _raw(eng, bgr, packed, vert_ptr=vp, verts=verts, capacity=n, q=0)
    _raw(eng, bgr, packed, b=0, img=None, a=None, pp=None, pc=None, ip=None, vp=None)
    _raw(eng, bgr, packed, q=0, img=None, a=None, pp=None, pc=None, ip=None, vp=None, h=0)
    assert bool((vp == POISON).all()) and bool((verts == POISON).all())


def test_refusals(eng):
    from gcn_grabcut import _native
    h, w = 40, 1100
    bgr = torch.zeros((2, h, w, 3), dtype=torch.uint8, device=eng.device)
    vp = torch.full((3,), POISON, dtype=torch.int32, device=eng.device)
    verts = torch.full((64, 2), POISON, dtype=torch.int32, device=eng.device)

    def packed(anchors=((1, 1), (5, 9), (9, 2), (0, 0), (3, 3)), pp=(0, 3, 5), pc=(1, 0), ip=(0, 1, 2)):
        return eng.upload_paths(np.array(anchors, np.int32).reshape(-1, 2), list(pp), list(pc), list(ip))

    def refused(code, pk=None, **kw):
        with pytest.raises(_native.GGCError, match=code) as e:
            _raw(eng, bgr, pk or packed(), **{**dict(vert_ptr=vp, verts=verts, capacity=64), **kw})
        assert str(e.value).split(": ", 1)[1].strip(), kw               # with a message from ggc_last_error

    _raw(eng, bgr, packed(), vert_ptr=vp, verts=verts, capacity=64)     # the well-formed call is accepted ...
    assert int(vp[0]) == 0 and int(vp[2]) > 0
    vp.fill_(POISON)
    verts.fill_(POISON)
    for kw in (dict(h=0), dict(w=0), dict(h=65536), dict(w=65536), dict(b=65536), dict(b=-1)):
        refused("SHAPE", **kw)
    for kw in (dict(margin=-1), dict(margin=257), dict(edge_cap=0), dict(edge_cap=13771), dict(smooth=0), dict(smooth=65),
               dict(q=-1), dict(capacity=-1)):
        refused("INVALID_ARG", **kw)
    for name in ("img", "a", "pp", "pc", "ip", "vp"):
        refused("INVALID_ARG", **{name: None})
    for ip in ((1, 1, 2), (0, 2, 1), (0, 1, 1), (0, 1, 3)):             # not from 0; decreasing; not ending at Q
        refused("INVALID_ARG", packed(ip=ip))
    for pp in ((1, 3, 5), (0, 4, 3), (0, 5, 5), (0, 4, 5)):             # not from 0; decreasing; empty; an open path of one anchor
        refused("INVALID_ARG", packed(pp=pp))
    refused("INVALID_ARG", packed(pp=(0, 2, 5), pc=(1, 1)))             # a closed path of two anchors
    refused("INVALID_ARG", packed(pc=(1, 2)))                           # path_closed outside {0, 1}
    for bad in ((-1, 1), (1, -1), (h, 1), (1, w)):                      # an anchor outside its image
        refused("INVALID_ARG", packed(anchors=((1, 1), bad, (9, 2), (0, 0), (3, 3))))
    refused("INVALID_ARG", packed(anchors=((1, 1), (5, 9), (9, 2), (0, 0), (3, 1025))))        # more than 1024 apart
    refused("INVALID_ARG", packed(anchors=((1, 1), (5, 9), (9, 1026), (0, 0), (3, 3))))        # ... the closing segment counts
    assert bool((vp == POISON).all()) and bool((verts == POISON).all())                        # refused before any launch
    # windows that hold more than 2^26 pixels in all: 2^12 open paths of 1025 x 40 pixels and margin 256
    many = 1 << 12
    a = np.tile(np.array([[0, 0], [39, 1024]], np.int32), (many, 1))
    big = eng.upload_paths(a, np.arange(0, 2 * many + 1, 2), np.zeros(many), [0, many, many])
    vp_big = torch.full((many + 1,), POISON, dtype=torch.int32, device=eng.device)
    with pytest.raises(_native.GGCError, match="INVALID_ARG"):
        _raw(eng, bgr, big, setting=(256, 2048, 16), vert_ptr=vp_big)
    assert bool((vp_big == POISON).all())


# ---------------------------------------------------------------- through the painter

def test_traced_batch_goes_straight_into_the_painter(eng, kernel_batch):
    from gcn_grabcut.graph_builder import pack_paths
    imgs, paths = kernel_batch
    closed = [[p for p in (ps or []) if p[1]] for ps in paths]
    want_v, want_p = ref.trace_batch(imgs, closed, *DEFAULTS)
    assert (np.diff(want_p) >= 3).all()
    a, pp, pc, ip = pack_paths([[(x, True) for x, _ in ps] or None for ps in closed])
    d = eng.upload_paths(a, pp, pc, ip)
    verts, vert_ptr = eng.trace_paths(eng.to_device(np.stack(imgs)), *d, *DEFAULTS)
    labels = torch.full((len(pc),), 2, dtype=torch.int32, device=eng.device)           # every traced outline a lasso
    masks = np.full((6, H0, W0), 3, np.uint8)
    got = eng.apply_polygons(eng.to_device(masks), verts, vert_ptr, labels, d[3]).cpu().numpy()
    want = polygons_ref.apply_packed(masks, want_v, want_p, np.full(len(pc), 2, np.int32), ip, covered=polygons_ref.covered_np)
    assert np.array_equal(got, want)
    assert (got[1] == 3).all() and (got[0] == 0).any() and (got[0] == 3).any()


# ---------------------------------------------------------------- pipeline

H, W = 96, 128
KEYS = ("binary_mask", "trimap", "segments", "probs", "gc_mask", "overlay", "rgba")


@pytest.fixture(scope="module")
def scene():
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig
    from gcn_grabcut.synthetic import synthetic_image
    model, sd = seeded_state_dict(32, 2, seed=5)
    pipe = GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=80), device="cuda")
    data = [synthetic_image(H, W, 30000 + i, return_mask=True) for i in range(3)]
    anchors = [ref.boundary_anchors(gt, 6)[1] for _, gt in data]
    return pipe, [img for img, _ in data], anchors


def test_public_trace_boundary(scene):
    from gcn_grabcut import Scissors, trace_boundary
    pipe, imgs, anchors = scene
    got = trace_boundary(imgs[0], anchors[0])
    assert got.dtype == np.int32 and np.array_equal(got, ref.trace_path(imgs[0], anchors[0], True, *DEFAULTS))
    opt = Scissors(margin=4, edge_cap=512, smooth=3)
    assert np.array_equal(trace_boundary(imgs[0], anchors[0][:3], closed=False, scissors=opt),
                          ref.trace_path(imgs[0], anchors[0][:3], False, 4, 512, 3))
    with pytest.raises(ValueError):
        trace_boundary(imgs[0], [(0, 0), (H, 5), (9, 9)])
    with pytest.raises(ValueError):
        trace_boundary(imgs[0], anchors[0][:2])


def test_segment_with_scissors_is_segment_with_the_traced_lasso(scene):
    from gcn_grabcut import Scissors, trace_boundary
    pipe, imgs, anchors = scene
    r = pipe.segment(imgs[0], scissors=anchors[0], min_area_ratio=0.0)
    lasso = trace_boundary(imgs[0], anchors[0])
    want = pipe.segment(imgs[0], lasso=lasso, min_area_ratio=0.0)
    assert np.array_equal(r.trimap, want.trimap) and np.array_equal(r.binary_mask, want.binary_mask)
    outside = ~polygons_ref.covered_np((H, W), [tuple(v) for v in lasso])
    assert outside.sum() > 1000 and (r.trimap[outside] == 0).all() and not r.binary_mask[outside].any()
    # options travel, several anchor lists form a union, and a lasso joins it
    opt = Scissors(margin=6, edge_cap=1024, smooth=8)
    two = [anchors[0][:3], anchors[0][3:]]
    r2 = pipe.segment(imgs[0], scissors=two, scissors_options=opt, lasso=[(0, 0), (0, 20), (20, 0)], min_area_ratio=0.0)
    traced = [trace_boundary(imgs[0], a, scissors=opt) for a in two]
    want2 = pipe.segment(imgs[0], lasso=traced + [[(0, 0), (0, 20), (20, 0)]], min_area_ratio=0.0)
    assert np.array_equal(r2.trimap, want2.trimap) and np.array_equal(r2.binary_mask, want2.binary_mask)
    with pytest.raises(ValueError):                                     # an outline of one pixel
        pipe.segment(imgs[0], scissors=[(5, 5), (5, 5), (5, 5)])
    with pytest.raises(ValueError):
        pipe.segment(imgs[0], scissors=anchors[0], scissors_options=(16, 2048, 16))


def test_segment_scissors_is_segment_lasso_on_the_traced_outline(scene):
    from gcn_grabcut import trace_boundary
    pipe, imgs, anchors = scene
    r = pipe.segment_scissors(imgs[1], anchors[1])
    want = pipe.segment_lasso(imgs[1], trace_boundary(imgs[1], anchors[1]))
    assert np.array_equal(r.trimap, want.trimap) and np.array_equal(r.binary_mask, want.binary_mask)
    assert (r.trimap == 3).any() and (r.trimap == 0).any()


def test_segment_batch_with_scissors_equals_single_calls(scene):
    pipe, imgs, anchors = scene
    per_image = [anchors[0], None, [anchors[2][:3], anchors[2][3:]]]
    res = pipe.segment_batch(imgs, scissors=per_image, min_area_ratio=0.0, chunks=1)
    plain = pipe.segment_batch(imgs, min_area_ratio=0.0, chunks=1)
    from gcn_grabcut import trace_boundary
    lassos = [([], [], [trace_boundary(imgs[0], anchors[0])]), None,
              ([], [], [trace_boundary(imgs[2], anchors[2][:3]), trace_boundary(imgs[2], anchors[2][3:])])]
    same = pipe.segment_batch(imgs, polygons=lassos, min_area_ratio=0.0, chunks=1)
    for i in range(3):
        assert np.array_equal(res[i].trimap, same[i].trimap) and np.array_equal(res[i].binary_mask, same[i].binary_mask), i
        one = pipe.segment_batch([imgs[i]], scissors=[per_image[i]], min_area_ratio=0.0, chunks=1)[0]
        assert np.array_equal(res[i].trimap, one.trimap), i
        if i == 0:                                                      # GrabCut seeds image b with seed + b: only image 0 keeps its seed alone
            assert np.array_equal(res[i].binary_mask, one.binary_mask)
    assert np.array_equal(res[1].trimap, plain[1].trimap) and np.array_equal(res[1].binary_mask, plain[1].binary_mask)
    assert not np.array_equal(res[0].trimap, plain[0].trimap)


def test_pipeline_scissors_chunked_equals_one_chunk(scene):
    pipe, imgs, anchors = scene
    four = pipe._eng.to_device(np.stack(imgs + imgs[:1]))
    per_image = [anchors[0], None, [anchors[2][:3], anchors[2][3:]], anchors[0][::-1]]
    one = pipe.segment_batch_device(four, chunks=1, min_area_ratio=0.0, scissors=per_image)
    two = pipe.segment_batch_device(four, chunks=2, min_area_ratio=0.0, scissors=per_image)
    for k in KEYS:
        assert torch.equal(one[k], two[k]), k


def test_without_scissors_none_of_the_new_kernels_is_launched(scene):
    pipe, imgs, anchors = scene
    ctx = pipe._eng.ctx
    names = ("scissors_guide", "scissors_round", "scissors_walk")
    ctx.profile_enable(1)
    try:
        pipe.segment(imgs[0], lasso=[(5, 5), (5, 100), (80, 60)], fg_points=[(40, 60)])
        pipe.segment_batch(imgs, scissors=[None, None, None])
        assert [ctx.profile_query(n)[0] for n in names] == [0, 0, 0]
        pipe.segment(imgs[0], scissors=anchors[0])
        launches = [ctx.profile_query(n)[0] for n in names]
        assert launches[0] >= 1 and launches[1] >= 1 and launches[2] >= 2        # the walk counts, then fills
    finally:
        ctx.profile_enable(0)


# ---------------------------------------------------------------- CLI

def test_cli_takes_scissors(tmp_path):
    from PIL import Image
    from gcn_grabcut import trace_boundary
    from gcn_grabcut.synthetic import synthetic_image
    img, gt = synthetic_image(150, 200, 30003, return_mask=True)
    Image.fromarray(img[:, :, ::-1]).save(tmp_path / "x.png")
    model, sd = seeded_state_dict(32, 2, seed=8)
    torch.save({"model": sd, "epoch": 1}, tmp_path / "ckpt.pt")
    _, anchors = ref.boundary_anchors(gt, 6)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--image", str(tmp_path / "x.png"), "--output", str(out),
                        "--checkpoint", str(tmp_path / "ckpt.pt"), "--superpixels", "100", "--max-size", "200",
                        "--min-area", "0", "--save", "mask", "--scissors", " ".join(f"{r},{c}" for r, c in anchors),
                        "--scissors-margin", "12", "--scissors-edge-cap", "1024", "--scissors-smooth", "8"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    mask = np.asarray(Image.open(out / "x_mask.png"))
    assert mask.shape == (150, 200)
    from gcn_grabcut import Scissors
    lasso = trace_boundary(img, anchors, scissors=Scissors(12, 1024, 8))
    outside = ~polygons_ref.covered_np((150, 200), [tuple(v) for v in lasso])
    assert outside.sum() > 2000 and (mask[outside] == 0).all() and mask.any()
