"""Lassos and filled polygons on the host: properties of the polygon rule's restatement (tests/polygons_ref.py), packing
per-image polygons for ggc_apply_polygons, their chunking, the header / ctypes entries, and the CLI's polygon flags."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import polygons_ref as ref
from gcn_grabcut import paint_polygons, polygon_mask  # noqa: F401  (the feature under test: without it nothing here runs)
from gcn_grabcut.graph_builder import pack_polygons

ROOT = Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------- the rule

def _hull(points):
    """Strict convex hull (monotone chain, no collinear vertex) of integer points, as a list of (row, col)."""
    pts = sorted(set(points))

    def half(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and (out[-1][0] - out[-2][0]) * (p[1] - out[-2][1]) - (out[-1][1] - out[-2][1]) * (p[0] - out[-2][0]) <= 0:
                out.pop()
            out.append(p)
        return out[:-1]
    return half(pts) + half(pts[::-1])


def _half_planes(shape, poly, origin=(0, 0)):
    """Convex polygon: p is covered iff every edge cross product has one sign (or is zero)."""
    out = np.zeros(shape, bool)
    n = len(poly)
    for r in range(shape[0]):
        for c in range(shape[1]):
            pr, pc = r + origin[0], c + origin[1]
            cr = [(poly[(i + 1) % n][0] - poly[i][0]) * (pc - poly[i][1]) - (poly[(i + 1) % n][1] - poly[i][1]) * (pr - poly[i][0])
                  for i in range(n)]
            out[r, c] = all(v >= 0 for v in cr) or all(v <= 0 for v in cr)
    return out


def _random_polygon(rng, n, lo, hi):
    return [(int(rng.integers(lo, hi)), int(rng.integers(lo, hi))) for _ in range(n)]


def test_rectangle_is_the_inclusive_box():
    rng = np.random.default_rng(1)
    for _ in range(30):
        r0, r1 = sorted(int(v) for v in rng.integers(-3, 16, 2))
        c0, c1 = sorted(int(v) for v in rng.integers(-3, 16, 2))
        yy, xx = np.mgrid[0:12, 0:13]
        box = (yy >= r0) & (yy <= r1) & (xx >= c0) & (xx <= c1)
        assert np.array_equal(ref.covered((12, 13), [(r0, c0), (r0, c1), (r1, c1), (r1, c0)]), box)


def test_convex_hulls_match_the_half_plane_definition():
    rng = np.random.default_rng(2)
    done = 0
    while done < 60:
        hull = _hull(_random_polygon(rng, int(rng.integers(3, 10)), -2, 16))
        if len(hull) < 3:
            continue
        done += 1
        assert np.array_equal(ref.covered((14, 14), hull), _half_planes((14, 14), hull)), hull


def test_invariance_under_reversal_rotation_translation_and_transposition():
    rng = np.random.default_rng(3)
    for _ in range(40):                                                   # self-intersecting as a rule
        poly = _random_polygon(rng, int(rng.integers(3, 9)), -3, 15)
        want = ref.covered((12, 12), poly)
        assert np.array_equal(ref.covered((12, 12), poly[::-1]), want), poly
        k = int(rng.integers(1, len(poly)))
        assert np.array_equal(ref.covered((12, 12), poly[k:] + poly[:k]), want), poly
        dr, dc = int(rng.integers(-50, 50)), int(rng.integers(-50, 50))
        assert np.array_equal(ref.covered((12, 12), [(r + dr, c + dc) for r, c in poly], origin=(dr, dc)), want), poly
        assert np.array_equal(ref.covered((12, 12), [(c, r) for r, c in poly]), want.T), poly


def test_bow_tie_covers_its_lobes_and_crossing_but_not_its_notches():
    m = ref.covered((9, 9), [(0, 0), (0, 8), (8, 0), (8, 8)])
    assert m[4, 4] and m[1, 4] and m[7, 4] and m[0].all() and m[8].all()
    assert not m[4, 1] and not m[4, 7] and not m[3, 0] and not m[5, 8]
    assert m[4].sum() == 1                                                # the crossing point alone
    yy, xx = np.mgrid[0:9, 0:9]
    assert np.array_equal(m, (np.abs(xx - 4) <= np.abs(yy - 4)))


def test_ray_through_a_vertex_counts_once():
    diamond = [(0, 4), (4, 8), (8, 4), (4, 0)]
    m = ref.covered((9, 11), diamond, origin=(0, -1))
    assert m[0].sum() == 1 and m[0, 5] and m[8].sum() == 1               # an apex row holds exactly one pixel
    assert m[4].tolist() == [False] + [True] * 9 + [False]               # the row through two vertices
    yy, xx = np.mgrid[0:9, -1:10]
    assert np.array_equal(m, np.abs(yy - 4) + np.abs(xx - 4) <= 4)
    # a spike whose tip lies on the ray, right of the pixel: parity must not flip
    spike = [(0, 0), (0, 2), (3, 2), (2, 6), (5, 2), (8, 2), (8, 0)]
    m = ref.covered((9, 8), spike)
    assert m[2].tolist() == [True, True, True, False, False, False, True, False]     # the body, then the tip alone
    assert m[3].tolist() == [True, True, True, True, True, False, False, False]


def test_collinear_triples():
    box = ref.covered((8, 8), [(1, 1), (1, 6), (5, 6), (5, 1)])
    assert np.array_equal(ref.covered((8, 8), [(1, 1), (1, 3), (1, 6), (3, 6), (5, 6), (5, 2), (5, 1), (2, 1)]), box)
    flat = ref.covered((4, 12), [(0, 0), (0, 5), (0, 9)])                # zero area: its on-edge pixels only
    assert flat[0, :10].all() and flat.sum() == 10
    diag = ref.covered((8, 8), [(2, 2), (6, 6), (4, 4)])
    assert np.array_equal(diag, np.eye(8, dtype=bool) & (np.arange(8) >= 2)[:, None] & (np.arange(8) <= 6)[:, None])


def test_vertices_at_the_coordinate_limit():
    big = 2 ** 20
    tri = [(-big, -big), (-big, big), (big, 0)]
    assert ref.covered((8, 8), tri, origin=(-4, -4)).all()
    for origin in ((big - 6, -4), (-big - 2, big - 5), (0, big // 2 - 4), (1, -big // 2 - 4)):
        assert np.array_equal(ref.covered((8, 8), tri, origin), _half_planes((8, 8), tri, origin)), origin
    # the largest product of the rule: a full-span edge against a pixel at the far corner stays below 2^44
    assert abs((2 * big) * (2 * big + 65535)) < 2 ** 44


def test_the_vectorised_restatement_equals_the_scalar_one():
    rng = np.random.default_rng(4)
    for _ in range(40):
        poly = _random_polygon(rng, int(rng.integers(3, 9)), -4, 18)
        assert np.array_equal(ref.covered_np((13, 15), poly, (-1, -2)), ref.covered((13, 15), poly, (-1, -2))), poly
    big = 2 ** 20
    for poly in ([(-big, -big), (-big, big), (big, 0)], [(big, big), (-big, -big), (big, -big), (-big, big)]):
        for origin in ((big - 6, -4), (-4, -4), (-big - 2, big - 5), (0, big // 2 - 4)):
            assert np.array_equal(ref.covered_np((8, 8), poly, origin), ref.covered((8, 8), poly, origin)), (poly, origin)


def test_lassos_form_a_union_and_the_last_fill_wins():
    start = np.full((10, 12), 7, np.uint8)
    a, b = [(1, 1), (1, 4), (4, 4), (4, 1)], [(6, 7), (6, 10), (8, 10), (8, 7)]
    out = ref.apply(start, [(ref.LASSO, a), (ref.LASSO, b)])
    inside = ref.covered((10, 12), a) | ref.covered((10, 12), b)
    assert (out[inside] == 7).all() and (out[~inside] == ref.BGD).all()
    f1, f2 = [(0, 0), (0, 6), (6, 6), (6, 0)], [(3, 3), (3, 9), (9, 9), (9, 3)]
    out = ref.apply(start, [(ref.FG_FILL, f1), (ref.BG_FILL, f2)])
    assert out[1, 1] == ref.FGD and out[4, 4] == ref.BGD and out[8, 8] == ref.BGD and out[9, 0] == 7
    out = ref.apply(start, [(ref.BG_FILL, f2), (ref.FG_FILL, f1)])
    assert out[4, 4] == ref.FGD and out[8, 8] == ref.BGD
    out = ref.apply(start, [(ref.FG_FILL, f2), (ref.LASSO, a)])           # fills come after lassos whatever the order given
    assert out[8, 8] == ref.FGD and out[0, 11] == ref.BGD and out[2, 2] == 7


# ---------------------------------------------------------------- packing

def test_pack_polygons_orders_lassos_then_foreground_then_background():
    tri, quad, las = [(0, 0), (0, 5), (5, 0)], [(1, 1), (1, 3), (3, 3), (3, 1)], [(-9, -9), (-9, 40), (40, 40), (40.7, -9.7)]
    verts, pp, pl, ip = pack_polygons([None, ([tri], [quad, tri], [las]), None, ([], [], []), ([quad], [], [])])
    assert all(a.dtype == np.int32 for a in (verts, pp, pl, ip))
    assert ip.tolist() == [0, 0, 4, 4, 4, 5]
    assert pl.tolist() == [2, 1, 0, 0, 1]
    assert pp.tolist() == [0, 4, 7, 11, 14, 18]
    assert verts.tolist() == [list(p) for p in [(-9, -9), (-9, 40), (40, 40), (40, -9)] + tri + quad + tri + quad]
    empty = pack_polygons([None, None])
    assert [a.shape for a in empty] == [(0, 2), (1,), (0,), (3,)] and empty[3].tolist() == [0, 0, 0]
    far = pack_polygons([([[(2**20, -2**20), (0, 0), (-2**20, 2**20)]], [], [])])
    assert far[0].tolist() == [[2**20, -2**20], [0, 0], [-2**20, 2**20]]


@pytest.mark.parametrize("bad", [
    [([[(1, 2), (3, 4)]], [], [])],                 # two vertices
    [([[]], [], [])],                               # an empty polygon
    [([[(1, 2, 3), (1, 2, 3), (1, 2, 3)]], [], [])],
    [([(1, 2), (3, 4), (5, 6)], [], [])],           # a polygon's vertices given where the list of polygons belongs
    [([], [])],                                     # a pair, not a triple
    ["abc"],
    [(["abc"], [], [])],
    [([], [], "abc")],
    [([[(float("nan"), 2), (0, 0), (1, 1)]], [], [])],
    [([], [], [[(2**20 + 1, 0), (0, 0), (1, 5)]])],  # beyond the kernel's coordinate limit
])
def test_pack_polygons_rejects_bad_shapes(bad):
    with pytest.raises(ValueError):
        pack_polygons(bad)


def test_lasso_argument_is_one_polygon_or_a_list():
    from gcn_grabcut.graph_builder import lasso_list
    tri, quad = [(0, 0), (0, 5), (5, 0)], [(1, 1), (1, 3), (3, 3), (3, 1)]
    assert lasso_list(None) == [] and lasso_list(tri) == [tri] and lasso_list(np.array(tri)) [0].tolist() == [list(p) for p in tri]
    assert lasso_list([tri, quad]) == [tri, quad] and lasso_list([tri, tri]) == [tri, tri]
    with pytest.raises(ValueError):
        lasso_list("1,2 3,4 5,6")


def test_hints_carry_and_chunk_polygons():
    from gcn_grabcut.pipeline import _Hints
    tri, quad = [(0, 0), (0, 5), (5, 0)], [(1, 1), (1, 3), (3, 3), (3, 1)]
    assert _Hints.of(None, 3, 5, False, False, polygons=None) is None
    assert _Hints.of(None, 3, 5, False, False, polygons=[None, ([], [], []), None]) is None
    h = _Hints.of(None, 4, 5, False, False, polygons=[None, ([tri], [], [quad]), None, ([], [quad, tri], [])])
    assert h.rows.shape == (0, 3) and h.segs is None and not h.has_clicks
    verts, pp, pl, ip = h.polys
    assert ip.tolist() == [0, 0, 2, 2, 4] and pl.tolist() == [2, 1, 0, 0] and pp.tolist() == [0, 4, 7, 11, 14]
    assert h.chunk(0, 1) is None and h.chunk(2, 3) is None                # no click, stroke or polygon in the chunk
    c = h.chunk(1, 3)
    assert c.polys[3].tolist() == [0, 2, 2] and c.polys[2].tolist() == [2, 1] and c.polys[1].tolist() == [0, 4, 7]
    assert c.polys[0].tolist() == [list(p) for p in quad + tri]
    c = h.chunk(2, 4)
    assert c.polys[3].tolist() == [0, 0, 2] and c.polys[2].tolist() == [0, 0] and c.polys[1].tolist() == [0, 4, 7]
    assert c.polys[0].tolist() == [list(p) for p in quad + tri]
    whole = h.chunk(0, 4)
    assert all(np.array_equal(a, b) for a, b in zip(whole.polys, h.polys))
    packed = _Hints.of(None, 4, 5, False, False, polygons=h.polys)        # the packed form is accepted as it is
    assert all(np.array_equal(a, b) for a, b in zip(packed.polys, h.polys))
    clicks = _Hints.of([None, ([(1, 1)], []), None, None], 4, 5, False, False, polygons=[None, None, None, ([tri], [], [])])
    assert clicks.has_clicks and clicks.chunk(0, 2).polys is None and clicks.chunk(2, 4).polys is not None
    assert not clicks.chunk(2, 4).has_clicks
    only_clicks = _Hints.of([None, ([(1, 1)], []), None, None], 4, 5, False, False)
    assert only_clicks.polys is None and only_clicks.chunk(0, 4).polys is None
    with pytest.raises(ValueError):
        _Hints.of(None, 3, 5, False, False, polygons=[None, None])       # wrong length
    with pytest.raises(ValueError):
        _Hints.of(None, 3, 5, False, False, polygons=h.polys)            # packed for four images


# ---------------------------------------------------------------- ABI

def test_header_and_table_carry_the_polygon_entry():
    from gcn_grabcut import _native
    header = (ROOT / "include" / "ggc.h").read_text()
    assert int(re.search(r"#define GGC_VERSION (\d+)", header).group(1)) >= 406
    assert "ggc_apply_polygons" in header and "H3" in header
    for phrase in ("(a.r <= r) != (b.r <= r)", "(hi.c - lo.c)(r - lo.r) - (c - lo.c)(hi.r - lo.r) > 0", "SYNCHRONISES"):
        assert phrase in header[header.index("/* H3"):header.index("int ggc_apply_polygons")]
    assert len(_native.SIGNATURES["ggc_apply_polygons"]) == 11


def test_public_names():
    import gcn_grabcut
    for name in ("pack_polygons", "paint_polygons", "polygon_mask"):
        assert name in gcn_grabcut.__all__ and callable(getattr(gcn_grabcut, name))
    for name in ("add_polygons", "run_with_lasso"):
        assert hasattr(gcn_grabcut.GrabCut, name)
    assert hasattr(gcn_grabcut.GCNGrabCutPipeline, "segment_lasso")


# ---------------------------------------------------------------- CLI

def test_cli_refuses_polygons_on_a_folder(tmp_path):
    for flag in ("--lasso", "--fg-polygon", "--bg-polygon"):
        r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--input", str(tmp_path), flag, "3,4 5,6 9,1"],
                           cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2, (flag, r.stderr)
        assert "--lasso / --fg-polygon / --bg-polygon are polygons on one image" in r.stderr, (flag, r.stderr)


def test_cli_parses_and_scales_polygon_vertices():
    sys.path.insert(0, str(ROOT))
    import inference
    args = inference.build_parser().parse_args(["--image", "x.png", "--lasso", "100,150 299,399 -4,400",
                                                "--bg-polygon", "7,8 9,10 11,12", "--bg-polygon", "0,0 0,9 9,9 9,0",
                                                "--fg-polygon", "1,2 3,4 5,7"])
    assert args.lasso == [(100, 150), (299, 399), (-4, 400)]
    assert args.bg_polygon == [[(7, 8), (9, 10), (11, 12)], [(0, 0), (0, 9), (9, 9), (9, 0)]]
    assert args.fg_polygon == [[(1, 2), (3, 4), (5, 7)]]
    assert inference.scale_points(args.lasso, (300, 400), (150, 200)) == [(50, 75), (149, 199), (-2, 200)]
    none = inference.build_parser().parse_args(["--image", "x.png"])
    assert none.lasso is None and none.fg_polygon == [] and none.bg_polygon == []
    for bad in ("1,2 3,4", "1,2 3,4 5", ""):
        with pytest.raises(SystemExit):
            inference.build_parser().parse_args(["--image", "x.png", "--lasso", bad])
