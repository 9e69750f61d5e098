"""Lassos and filled polygons on the MI355X: ggc_apply_polygons against the integer restatement of its rule
(tests/polygons_ref.py), then the pipeline with polygons (hard constraints, untouched neighbours, chunked runs, clicks over
excluded areas), segment_lasso, GrabCut.add_polygons + refine, and the CLI's --lasso."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import polygons_ref as ref
from helpers import seeded_state_dict

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
POISON = 7


@pytest.fixture(scope="module")
def eng():
    from gcn_grabcut._engine import get_engine
    return get_engine("cuda")


def _apply(eng, masks, packed):
    """ggc_apply_polygons through ctx.call on a (B,H,W) uint8 batch; packed = pack_polygons' four host arrays."""
    verts, pp, pl, ip = eng.upload_polygons(*packed)
    m = eng.to_device(np.ascontiguousarray(masks))
    b, h, w = m.shape
    eng.ctx.call("ggc_apply_polygons", eng._stream(), b, h, w, verts.data_ptr(), pp.data_ptr(), pl.data_ptr(), ip.data_ptr(),
                 len(packed[2]), m.data_ptr())
    return m.cpu().numpy()


H0, W0 = 37, 53      # no multiple of the 32x8 tile: partial tiles on both borders, 2 x 5 tiles


def _base_batch():
    """B = 3: image 0 a concave 9-vertex lasso with two vertices outside the image plus overlapping fg and bg fills, image 1
    nothing, image 2 two disjoint lassos and a self-intersecting fill."""
    lasso9 = [(2, 3), (-6, 25), (4, 48), (18, 40), (12, 26), (30, 30), (44, 12), (33, 2), (16, 12)]
    fg, bg = [(5, 5), (5, 30), (25, 30), (25, 5)], [(15, 20), (10, 45), (34, 50), (36, 22)]
    las_a, las_b = [(1, 1), (1, 20), (14, 20), (14, 1)], [(20, 30), (20, 52), (36, 52), (36, 41), (28, 30)]
    bow = [(3, 3), (3, 49), (33, 3), (33, 49)]
    return [([fg], [bg], [lasso9]), None, ([bow], [], [las_a, las_b])]


def test_apply_polygons_matches_the_restatement(eng):
    from gcn_grabcut.graph_builder import pack_polygons
    per_image = _base_batch()
    packed = pack_polygons(per_image)
    masks = np.full((3, H0, W0), POISON, np.uint8)            # poison: an untouched pixel is neither read nor written
    got = _apply(eng, masks, packed)
    want = ref.apply_packed(masks, *packed, covered=ref.covered)
    assert np.array_equal(got, want)
    assert (got[1] == POISON).all()
    assert (got[0] == POISON).any() and (got[0] == 0).any() and (got[0] == 1).any()
    assert (got[2] == POISON).any() and (got[2] == 0).any() and (got[2] == 1).any()
    # the batch equals the three single-image calls
    for b in range(3):
        one = pack_polygons([per_image[b]])
        if len(one[2]) == 0:
            continue
        assert np.array_equal(_apply(eng, masks[b:b + 1], one)[0], got[b]), b
    # on random labels too: only the covered pixels change
    rnd = np.random.default_rng(5).integers(0, 4, (3, H0, W0)).astype(np.uint8)
    assert np.array_equal(_apply(eng, rnd, packed), ref.apply_packed(rnd, *packed))


def test_apply_polygons_label_order_is_by_index(eng):
    """Lassos anywhere in the list act first; of two overlapping fills the later wins, whatever their labels."""
    a, b = [(0, 0), (0, 30), (20, 30), (20, 0)], [(10, 10), (10, 50), (36, 50), (36, 10)]
    las = [(5, 5), (5, 45), (30, 45), (30, 5)]
    for labels, polys in (([0, 1, 2], [a, b, las]), ([1, 2, 0], [b, las, a]), ([2, 0, 1], [las, b, a])):
        verts = np.array([v for p in polys for v in p], np.int32)
        pp = np.cumsum([0] + [len(p) for p in polys]).astype(np.int32)
        packed = (verts, pp, np.array(labels, np.int32), np.array([0, 3], np.int32))
        masks = np.full((1, H0, W0), POISON, np.uint8)
        assert np.array_equal(_apply(eng, masks, packed), ref.apply_packed(masks, *packed)), labels


def test_apply_polygons_more_edges_than_one_streaming_pass(eng):
    """16x600 with a 300-vertex zig-zag: the polygon spans the 256-edge pass, and its edges lie right of most tiles."""
    h, w = 16, 600
    zig = [(-3 if i % 2 == 0 else 19, 2 * i) for i in range(300)]
    small = [(4, 100), (4, 140), (12, 140), (12, 100)]
    verts = np.array(zig + small, np.int32)
    packed = (verts, np.array([0, 300, 304], np.int32), np.array([1, 0], np.int32), np.array([0, 2], np.int32))
    masks = np.full((1, h, w), POISON, np.uint8)
    got = _apply(eng, masks, packed)
    assert np.array_equal(got, ref.apply_packed(masks, *packed))
    assert (got == 1).sum() > 1000 and (got == POISON).sum() > 1000 and (got[0, 4:13, 100:141] == 0).all()
    lasso = (verts[:300], np.array([0, 300], np.int32), np.array([2], np.int32), np.array([0, 1], np.int32))
    assert np.array_equal(_apply(eng, masks, lasso), ref.apply_packed(masks, *lasso))


def test_apply_polygons_degenerate_cases(eng):
    from gcn_grabcut.graph_builder import pack_polygons
    masks = np.full((2, H0, W0), POISON, np.uint8)
    outside = [(-30, -30), (-30, -5), (-8, -5), (-8, -30)]
    got = _apply(eng, masks, pack_polygons([([], [], [outside]), ([outside], [outside], [])]))
    assert (got[0] == 0).all() and (got[1] == POISON).all()   # a lasso off the image: all background; a fill: nothing
    flat = [(3, 2), (20, 36), (11.0, 18)]                     # zero area: a segment walked there and back
    got = _apply(eng, masks[:1], pack_polygons([([flat], [], [])]))
    want = ref.apply_packed(masks[:1], *pack_polygons([([flat], [], [])]), covered=ref.covered)
    assert np.array_equal(got, want)
    assert sorted(zip(*np.nonzero(got[0] == 1))) == [(3 + k, 2 + 2 * k) for k in range(18)]   # its lattice points: gcd(17, 34) = 17
    far = [(2**20, -2**20), (-2**20, -2**20), (0, 2**20)]     # the limits themselves
    got = _apply(eng, masks[:1], pack_polygons([([far], [], [])]))
    assert (got == 1).all()
    edge = [(2**20, 40), (-2**20, 10), (-2**20, 2**20)]       # a full-span edge through the image
    packed = pack_polygons([([], [edge], [])])
    assert np.array_equal(_apply(eng, masks[:1], packed), ref.apply_packed(masks[:1], *packed, covered=ref.covered))


def test_apply_polygons_no_ops_and_refusals(eng):
    from gcn_grabcut import _native
    h, w = 9, 11
    mask = torch.full((2, h, w), POISON, dtype=torch.uint8, device=eng.device)
    st = eng._stream()
    tri = np.array([[1, 1], [1, 7], [6, 4]], np.int32)
    good = eng.upload_polygons(tri, [0, 3], [1], [0, 1, 1])

    def call(b=2, hh=h, ww=w, verts=good[0], pp=good[1], pl=good[2], ip=good[3], n=1, m=mask):
        return eng.ctx.call("ggc_apply_polygons", st, b, hh, ww, _native.ptr(verts), _native.ptr(pp), _native.ptr(pl),
                            _native.ptr(ip), n, _native.ptr(m))

    def refused(code, **kw):
        with pytest.raises(_native.GGCError, match=code) as e:
            call(**kw)
        assert str(e.value).split(": ", 1)[1].strip(), kw               # with a message from ggc_last_error

    call(b=0)                                                           # the no-ops write nothing
    call(n=0)
    call(b=0, verts=None, pp=None, pl=None, ip=None, m=None)
    call(n=0, verts=None, pp=None, pl=None, ip=None, m=None)
    assert bool((mask == POISON).all())
    refused("SHAPE", hh=0)
    refused("SHAPE", ww=65536)
    refused("SHAPE", b=65536)
    refused("SHAPE", b=-1)
    refused("SHAPE", b=-1, n=0)                                         # P == 0 is a no-op only after the shape check
    refused("SHAPE", hh=0, n=0)
    call(b=0, hh=0, n=-1)                                               # B == 0 is one whatever else is given
    refused("INVALID_ARG", n=-1)
    refused("INVALID_ARG", m=None)
    refused("INVALID_ARG", ip=None)
    refused("INVALID_ARG", pp=None)
    refused("INVALID_ARG", pl=None)
    refused("INVALID_ARG", verts=None)
    two = np.concatenate([tri, tri + 1])

    def packed(verts=two, pp=(0, 3, 6), pl=(1, 0), ip=(0, 1, 2)):
        v, p, l, i = eng.upload_polygons(verts, list(pp), list(pl), list(ip))
        return dict(verts=v, pp=p, pl=l, ip=i, n=len(pl))
    call(**packed())                                                    # the well-formed pair of polygons is accepted ...
    assert bool((mask[0] == 1).any()) and bool((mask[1] == 0).any())
    mask.fill_(POISON)
    for ip in ((1, 1, 2), (0, 2, 1), (0, 1, 1), (0, 1, 3)):             # not from 0; decreasing; not ending at P
        refused("INVALID_ARG", **packed(ip=ip))
    for pp in ((1, 3, 6), (0, 4, 3), (0, 6, 6)):                        # not from 0; decreasing; an empty polygon
        refused("INVALID_ARG", **packed(pp=pp))
    refused("INVALID_ARG", **packed(pp=(0, 2, 6)))                      # two vertices
    refused("INVALID_ARG", **packed(pp=(0, 4, 6)))
    for pl in ((1, 3), (-1, 0), (2, 256)):                              # a label outside {0, 1, 2}
        refused("INVALID_ARG", **packed(pl=pl))
    for j, v in ((0, 2**20 + 1), (5, -2**20 - 1), (7, 2**30)):          # a coordinate beyond +-2^20
        bad = two.copy()
        bad.ravel()[j] = v
        refused("INVALID_ARG", **packed(verts=bad))
    assert bool((mask == POISON).all())                                 # refused before any launch


def test_public_paint_polygons_and_polygon_mask():
    from gcn_grabcut import paint_polygons, polygon_mask
    fg, bg = [[(2, 2), (2, 30), (25, 16)]], [[(10, 10), (10, 50), (30, 50), (30, 10)]]
    lasso = [(0, 0), (0, 45), (36, 45), (36, 0)]
    m = np.random.default_rng(2).integers(0, 4, (H0, W0)).astype(np.uint8)
    polys = [(2, lasso), (1, fg[0]), (0, bg[0])]
    assert np.array_equal(paint_polygons(m, fg, bg, lasso), ref.apply(m, polys, ref.covered_np))
    assert np.array_equal(paint_polygons(m, fg, bg, [lasso]), ref.apply(m, polys, ref.covered_np))
    assert np.array_equal(paint_polygons((H0, W0), fg), ref.apply(np.full((H0, W0), 2, np.uint8), polys[1:2], ref.covered_np))
    assert np.array_equal(paint_polygons(m), m)
    bow = [(0, 0), (0, 8), (8, 0), (8, 8)]
    got = polygon_mask((9, 9), bow)
    assert got.dtype == np.uint8 and np.array_equal(got.astype(bool), ref.covered((9, 9), bow))
    with pytest.raises(ValueError):
        polygon_mask((9, 9), bow[:2])


# ---------------------------------------------------------------- pipeline

H, W = 96, 128
KEYS = ("binary_mask", "trimap", "segments", "probs", "gc_mask", "overlay", "rgba")
LASSO = [(10, 20), (4, 70), (20, 118), (70, 124), (92, 80), (60, 64), (88, 16), (50, 6)]     # concave
FG_POLY = [(40, 50), (40, 62), (52, 62), (52, 50)]
BG_POLY = [(46, 56), (46, 100), (58, 100), (58, 56)]                                         # overlaps FG_POLY: background wins


def _batch_polygons():
    return [([], [], [LASSO]), None, ([FG_POLY], [BG_POLY], [])]


@pytest.fixture(scope="module")
def polygon_runs():
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig
    from gcn_grabcut.synthetic import synthetic_batch
    model, sd = seeded_state_dict(32, 2, seed=5)
    pipe = GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=80), device="cuda")
    imgs = synthetic_batch(3, H, W, config_id=9)
    bgr = pipe._eng.to_device(imgs)
    polygons = _batch_polygons()
    kw = dict(chunks=1, min_area_ratio=0.0, return_state=True)
    base = pipe.segment_batch_device(bgr, **kw)
    cut = pipe.segment_batch_device(bgr, polygons=polygons, **kw)
    return pipe, imgs, bgr, polygons, base, cut


def test_pipeline_lasso_excludes_everything_outside(polygon_runs):
    pipe, imgs, bgr, polygons, base, cut = polygon_runs
    inside = ref.covered_np((H, W), LASSO)
    tri = cut["trimap"][0].cpu().numpy()
    want = base["trimap"][0].cpu().numpy().copy()
    want[~inside] = 0
    assert np.array_equal(tri, want)
    gc_mask = cut["gc_mask"][0].cpu().numpy()                           # GrabCut's own mask, before clean-up
    assert (gc_mask[~inside] == 0).all()
    assert (cut["gc_binary"][0].cpu().numpy()[~inside] == 0).all() and (cut["binary_mask"][0].cpu().numpy()[~inside] == 0).all()
    r = pipe.segment(imgs[0], lasso=LASSO, min_area_ratio=0.0)
    assert np.array_equal(r.trimap, tri) and np.array_equal(r.binary_mask, cut["binary_mask"][0].cpu().numpy())
    r = pipe.segment(imgs[0], lasso=[LASSO], min_area_ratio=0.0)        # a list of lassos is their union
    assert np.array_equal(r.trimap, tri)


def test_pipeline_fills_are_obeyed(polygon_runs):
    pipe, imgs, bgr, polygons, base, cut = polygon_runs
    fg, bg = ref.covered_np((H, W), FG_POLY), ref.covered_np((H, W), BG_POLY)
    fg &= ~bg
    assert fg.any() and bg.any()
    want = base["trimap"][2].cpu().numpy().copy()
    want[fg], want[bg] = 1, 0
    assert np.array_equal(cut["trimap"][2].cpu().numpy(), want)
    for k in ("gc_mask", "gc_binary", "binary_mask"):
        m = cut[k][2].cpu().numpy()
        assert (m[fg] == 1).all() and (m[bg] == 0).all(), k
    r = pipe.segment(imgs[2], fg_polygons=[FG_POLY], bg_polygons=[BG_POLY], min_area_ratio=0.0)
    assert np.array_equal(r.trimap, want) and np.array_equal(r.binary_mask, cut["binary_mask"][2].cpu().numpy())


def test_pipeline_polygons_leave_other_images_alone(polygon_runs):
    pipe, imgs, bgr, polygons, base, cut = polygon_runs
    for k in ("binary_mask", "trimap", "segments", "gc_mask", "gc_binary", "overlay", "rgba", "bgd", "fgd"):
        assert torch.equal(base[k][1], cut[k][1]), k
    assert torch.equal(base["probs"], cut["probs"])                     # areas do not touch the network or the prior
    assert torch.equal(base["graphs"].x, cut["graphs"].x)
    assert not torch.equal(base["trimap"][0], cut["trimap"][0]) and not torch.equal(base["trimap"][2], cut["trimap"][2])
    res = pipe.segment_batch(list(imgs), polygons=polygons, min_area_ratio=0.0, chunks=1)
    plain = pipe.segment_batch(list(imgs), min_area_ratio=0.0, chunks=1)
    assert np.array_equal(res[1].binary_mask, plain[1].binary_mask) and np.array_equal(res[1].trimap, plain[1].trimap)
    for b in range(3):
        assert np.array_equal(res[b].binary_mask, cut["binary_mask"][b].cpu().numpy()), b


def test_pipeline_polygons_chunked_equals_one_chunk(polygon_runs):
    pipe, imgs, bgr, polygons, base, cut = polygon_runs
    four = torch.cat([bgr, bgr[:1]])
    polys4 = polygons + [([], [BG_POLY], [])]
    one = pipe.segment_batch_device(four, chunks=1, min_area_ratio=0.0, polygons=polys4)
    two = pipe.segment_batch_device(four, chunks=2, min_area_ratio=0.0, polygons=polys4)
    for k in KEYS:
        assert torch.equal(one[k], two[k]), k
    for k in ("binary_mask", "trimap", "gc_mask"):
        assert torch.equal(one[k][:3], cut[k]), k


def test_pipeline_click_inside_an_excluded_area_wins(polygon_runs):
    pipe, imgs, bgr, polygons, base, cut = polygon_runs
    inside = ref.covered_np((H, W), LASSO)
    click = (90, 120)
    assert not inside[click[0] - 3:click[0] + 4, click[1] - 3:click[1] + 4].any()
    out = pipe.segment_batch_device(bgr, chunks=1, min_area_ratio=0.0, polygons=polygons, hints=[([click], []), None, None],
                                    hint_radius=3, return_state=True)
    yy, xx = np.mgrid[0:H, 0:W]
    disk = (yy - click[0]) ** 2 + (xx - click[1]) ** 2 <= 9
    want = cut["trimap"][0].cpu().numpy().copy()
    want[disk] = 1
    assert np.array_equal(out["trimap"][0].cpu().numpy(), want)
    gc_mask = out["gc_mask"][0].cpu().numpy()
    assert (gc_mask[disk] == 1).all() and (gc_mask[~inside & ~disk] == 0).all()
    stroke = [(86, 100), (86, 124)]                                     # and a stroke there, painted after the lasso too
    out = pipe.segment_batch_device(bgr, chunks=1, min_area_ratio=0.0, polygons=polygons, strokes=[([stroke], []), None, None],
                                    stroke_radius=1)
    assert (out["trimap"][0].cpu().numpy()[86, 100:125] == 1).all()


def test_pipeline_without_polygons_is_the_call_without_the_argument(polygon_runs):
    from gcn_grabcut.graph_builder import pack_polygons
    pipe, imgs, bgr, polygons, base, cut = polygon_runs
    for arg in (None, [None] * 3, [None, ([], [], []), ((), None, None)]):
        out = pipe.segment_batch_device(bgr, chunks=1, min_area_ratio=0.0, polygons=arg)
        for k in KEYS:
            assert torch.equal(out[k], base[k]), k
    packed = tuple(torch.from_numpy(a) for a in pack_polygons(polygons))   # the packed tuple equals the per-image lists
    out = pipe.segment_batch_device(bgr, chunks=1, min_area_ratio=0.0, polygons=packed)
    for k in KEYS:
        assert torch.equal(out[k], cut[k]), k
    # areas are not clicks: hint_region / hints_as_prior see none of them
    out = pipe.segment_batch_device(bgr, chunks=1, min_area_ratio=0.0, polygons=polygons, hint_region=True, hints_as_prior=True)
    for k in KEYS:
        assert torch.equal(out[k], cut[k]), k


# ---------------------------------------------------------------- segment_lasso, GrabCut

def test_segment_lasso_cuts_inside_the_lasso():
    from gcn_grabcut import GCNGrabCutPipeline, GrabCut
    from gcn_grabcut.synthetic import synthetic_image
    model, sd = seeded_state_dict(32, 2, seed=5)
    pipe = GCNGrabCutPipeline(model.eval(), device="cuda")
    img = synthetic_image(H, W, 1234)
    inside = ref.covered_np((H, W), LASSO)
    r = pipe.segment_lasso(img, LASSO)
    want = np.where(inside, 3, 0).astype(np.uint8)
    assert np.array_equal(r.trimap, want)                               # GC_PR_FGD inside, GC_BGD outside
    assert r.binary_mask.any() and not r.binary_mask[~inside].any()
    assert r.overlay.shape == img.shape and r.rgba.shape == (H, W, 4)
    gc = GrabCut(img, device="cuda")
    assert np.array_equal(gc.run_with_lasso(LASSO), r.binary_mask)
    assert np.array_equal(gc.lasso_trimap([LASSO[:4], LASSO[4:]]),
                          np.where(ref.covered_np((H, W), LASSO[:4]) | ref.covered_np((H, W), LASSO[4:]), 3, 0))
    soft = pipe.segment_lasso(img, LASSO, matte=True)
    assert np.array_equal(soft.binary_mask, r.binary_mask) and soft.alpha.shape == (H, W)
    with pytest.raises(ValueError):
        pipe.segment_lasso(img, LASSO[:2])


def test_grabcut_add_polygons_then_refine():
    from gcn_grabcut import GrabCut
    from gcn_grabcut.synthetic import synthetic_image
    img = synthetic_image(70, 90, 1234)
    gc = GrabCut(img, device="cuda")
    with pytest.raises(RuntimeError):
        gc.add_polygons(fg_polygons=[[(5, 5), (5, 9), (9, 9)]])
    tri = np.full((70, 90), 2, np.uint8)
    tri[20:50, 25:65] = 3
    tri[30:40, 35:55] = 1
    tri[:4] = 0
    gc.run_with_trimap(tri)
    m0 = gc.mask.copy()
    fg, bg = [[(55, 5), (55, 30), (66, 18)]], [[(25, 30), (45, 60), (45, 30)]]
    lasso = [(2, 2), (2, 80), (68, 80), (68, 2)]
    gc.add_polygons(fg_polygons=fg, bg_polygons=bg, lasso=lasso)
    want = ref.apply(m0, [(2, lasso), (1, fg[0]), (0, bg[0])], ref.covered_np)
    assert np.array_equal(gc.mask, want)
    assert gc.history[-1].tag == "polygons"
    binary = gc.refine(1)
    one = ref.covered_np((70, 90), fg[0])
    zero = (ref.covered_np((70, 90), bg[0]) | ~ref.covered_np((70, 90), lasso)) & ~one
    assert one.any() and zero.any()
    assert (gc.mask[one] == 1).all() and (gc.mask[zero] == 0).all()     # refine keeps the painted pixels
    assert (binary[one] == 1).all() and (binary[zero] == 0).all()


# ---------------------------------------------------------------- CLI

def test_cli_takes_a_lasso(tmp_path):
    from PIL import Image
    from gcn_grabcut.synthetic import synthetic_image
    img = synthetic_image(300, 400, 4242)
    Image.fromarray(img[:, :, ::-1]).save(tmp_path / "x.png")
    model, sd = seeded_state_dict(32, 2, seed=8)
    torch.save({"model": sd, "epoch": 1}, tmp_path / "ckpt.pt")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--image", str(tmp_path / "x.png"), "--output", str(out),
                        "--checkpoint", str(tmp_path / "ckpt.pt"), "--superpixels", "100", "--max-size", "200",
                        "--min-area", "0", "--save", "mask", "--lasso", "20,40 -10,300 280,380 200,180 290,30",
                        "--fg-polygon", "100,100 100,140 140,140 140,100"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    mask = np.asarray(Image.open(out / "x_mask.png"))
    assert mask.shape == (150, 200)                                     # the --max-size resize halved the image
    inside = ref.covered_np((150, 200), [(10, 20), (-5, 150), (140, 190), (100, 90), (145, 15)])
    fill = ref.covered_np((150, 200), [(50, 50), (50, 70), (70, 70), (70, 50)])
    assert (~inside).sum() > 2000 and (mask[~inside & ~fill] == 0).all() and (mask[fill] == 255).all()
