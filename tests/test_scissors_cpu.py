"""Intelligent scissors on the host: properties of the definition's restatement (tests/scissors_ref.py), the quality
condition on the study's scenes, packing per-image paths for ggc_trace_paths, joining traced outlines to a batch's polygons,
the header / ctypes entries and the CLI's --scissors flags."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import scissors_ref as ref
from gcn_grabcut import Scissors, trace_boundary  # noqa: F401  (the feature under test: without it nothing here runs)
from gcn_grabcut.graph_builder import pack_paths

ROOT = Path(__file__).resolve().parent.parent
DEFAULTS = (16, 2048, 16)


# ---------------------------------------------------------------- the definition

def test_distance_equals_scipy_dijkstra_on_the_explicit_window_graph():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (20, 27, 3)).astype(np.uint8)
    margin, edge_cap, smooth = 3, 2048, 16
    flat = ref.flatness(img, edge_cap)
    assert flat.min() >= 0 and flat.max() <= 255 and len(np.unique(flat)) > 20
    for a, b in (((2, 3), (15, 20)), ((19, 26), (0, 0)), ((10, 5), (10, 22))):
        (y0, x0, wh, ww), dist = ref.distance(flat, a, b, margin, smooth)
        rows, cols, costs = [], [], []
        for y in range(wh):
            for x in range(ww):
                for dy, dx, length in ref.DIRECTIONS:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < wh and 0 <= xx < ww:
                        rows.append(y * ww + x)
                        cols.append(yy * ww + xx)
                        costs.append(length * (smooth + int(flat[y0 + y, x0 + x]) + int(flat[y0 + yy, x0 + xx])))
        graph = coo_matrix((costs, (rows, cols)), shape=(wh * ww, wh * ww)).tocsr()
        want = dijkstra(graph, directed=True, indices=(b[0] - y0) * ww + (b[1] - x0))
        assert np.array_equal(dist.ravel(), want.astype(np.int64))       # symmetric costs: from b equals to b
        assert dist[b[0] - y0, b[1] - x0] == 0 and dist.max() < 1 << 27


def test_constant_image_paths_are_the_tie_rule():
    """F is 255 everywhere, so every path has max(|dr|, |dc|) pixels and its pixels are decided by the order N, NE, E, SE, S,
    SW, W, NW alone.  The sequences are worked out by hand."""
    img = np.full((12, 14, 3), 77, np.uint8)
    assert (ref.flatness(img, 2048) == 255).all() and (ref.flatness(img, 1) == 255).all()
    by_hand = [
        ((0, 0), (2, 5), 0, [(0, 0), (0, 1), (0, 2), (0, 3), (1, 4)]),      # E while E is still on a cheapest path, then SE
        ((2, 5), (0, 0), 0, [(2, 5), (2, 4), (2, 3), (2, 2), (1, 1)]),      # W comes before NW
        ((5, 0), (0, 0), 0, [(5, 0), (4, 0), (3, 0), (2, 0), (1, 0)]),
        ((0, 3), (3, 0), 0, [(0, 3), (1, 2), (2, 1)]),
        ((3, 3), (3, 7), 2, [(3, 3), (3, 4), (3, 5), (3, 6)]),
        ((6, 6), (2, 12), 4, [(6, 6), (5, 7), (4, 8), (3, 9), (2, 10), (2, 11)]),   # with room around it: NE before E
    ]
    for a, b, margin, want in by_hand:
        got = ref.trace_path(img, [a, b], False, margin, 2048, 16)
        assert len(got) == max(abs(a[0] - b[0]), abs(a[1] - b[1])) + 1
        assert [tuple(p) for p in got] == want + [b], (a, b)
    closed = ref.trace_path(img, [(1, 1), (1, 4), (4, 4)], True, 0, 2048, 16)
    assert [tuple(p) for p in closed] == [(1, 1), (1, 2), (1, 3), (1, 4), (2, 4), (3, 4), (4, 4), (3, 3), (2, 2)]
    assert len(ref.trace_path(img, [(3, 3), (3, 3)], False, 5, 2048, 16)) == 1       # equal anchors: the appended one alone


def test_path_follows_an_L_shaped_step_edge():
    """Distances are to the edge's pixels, the object's outermost pixels along the L, as the study measures them."""
    img = np.full((60, 60, 3), 40, np.uint8)
    img[20:, :40] = 200
    edge = np.zeros((60, 60), bool)
    edge[20, :40] = True
    edge[20:, 39] = True
    a, b = (20, 0), (59, 40)
    path = ref.trace_path(img, [a, b], False, *DEFAULTS)
    assert len(path) > 70
    assert ref.distance_to_boundary(edge, path).max() <= 1.0
    mid = np.array([[(a[0] + b[0]) // 2, (a[1] + b[1]) // 2]])
    assert ref.distance_to_boundary(edge, mid)[0] > 10                     # the chord cuts through the object


def test_the_window_bounds_the_path():
    img = np.full((40, 60, 3), 120, np.uint8)
    img[15:] = 20                                                         # a strong edge four rows below the anchors
    a, b = (10, 5), (10, 45)
    inside = ref.trace_path(img, [a, b], False, 0, 2048, 16)
    assert (inside[:, 0] == 10).all() and len(inside) == 41               # margin 0: the box is row 10
    free = ref.trace_path(img, [a, b], False, 16, 2048, 16)
    assert (free[:, 0] >= 14).sum() > 20                                  # with room, the detour along the edge is cheaper
    flat = ref.flatness(img, 2048)
    d0 = ref.distance(flat, a, b, 0, 16)[1]
    (y0, x0, _, _), d16 = ref.distance(flat, a, b, 16, 16)
    assert d16[a[0] - y0, a[1] - x0] < d0[0, 0]


def test_window_is_the_grown_box_clipped_to_the_image():
    assert ref.window((5, 9), (20, 3), 4, 30, 40) == (1, 0, 24, 14)
    assert ref.window((0, 0), (0, 0), 0, 1, 1) == (0, 0, 1, 1)
    assert ref.window((2, 2), (3, 3), 256, 37, 53) == (0, 0, 37, 53)
    assert len(ref.segments([(0, 0), (1, 1), (2, 2)], True)) == 3 and len(ref.segments([(0, 0), (1, 1), (2, 2)], False)) == 2
    assert ref.segments([(0, 0), (1, 1), (2, 2)], True)[-1] == ((2, 2), (0, 0))


def test_quality_on_the_study_scenes():
    """The quality condition: at the defaults the traced path's mean distance to the true boundary, averaged over the eight
    scenes, is below half the chords', for 4, 6 and 8 anchors.  The table is DESIGN.md §5.24's."""
    rows = ref.study_rows()
    table = {n: (round(tm, 2), round(cm, 2), round(tw, 1), round(cw, 1)) for n, tm, cm, tw, cw in rows}
    print(table)
    assert table == {4: (0.67, 3.78, 12.5, 18.8), 6: (0.46, 2.18, 5.4, 12.6), 8: (0.38, 1.23, 2.0, 10.2)}
    for n, tm, cm, _, _ in rows:
        assert tm < 0.5 * cm, (n, tm, cm)


# ---------------------------------------------------------------- packing, options

def test_pack_paths():
    tri, quad = [(0, 0), (0, 5), (5, 0)], [(1, 1), (1, 3), (3.9, 3.2), (3, 1)]
    a, pp, pc, ip = pack_paths([None, [tri, (quad[:2], False)], [], [(np.array(quad), True)]])
    assert all(x.dtype == np.int32 for x in (a, pp, pc, ip))
    assert ip.tolist() == [0, 0, 2, 2, 3] and pc.tolist() == [1, 0, 1] and pp.tolist() == [0, 3, 5, 9]
    assert a.tolist() == [list(p) for p in tri + quad[:2] + [(1, 1), (1, 3), (3, 3), (3, 1)]]
    assert pack_paths([[tri]], closed=False)[2].tolist() == [0]
    empty = pack_paths([None, None])
    assert [x.shape for x in empty] == [(0, 2), (1,), (0,), (3,)]
    for bad in ([[tri[:2]]], [[(tri[:1], False)]], [["abc"]], ["abc"], [[[(1, 2, 3)] * 3]], [[[(float("nan"), 1), (0, 0), (1, 1)]]], [5]):
        with pytest.raises(ValueError):
            pack_paths(bad)
    assert pack_paths([[tri[:2]]], closed=False)[1].tolist() == [0, 2]


def test_scissors_options_are_checked():
    s = Scissors()
    assert (s.margin, s.edge_cap, s.smooth) == DEFAULTS
    assert Scissors(0, 1, 1) and Scissors(256, 13770, 64)
    with pytest.raises(Exception):
        s.margin = 3                                                      # frozen
    for kw in (dict(margin=-1), dict(margin=257), dict(edge_cap=0), dict(edge_cap=13771), dict(smooth=0), dict(smooth=65),
               dict(margin=1.5), dict(smooth=True), dict(edge_cap="8")):
        with pytest.raises(ValueError):
            Scissors(**kw)


def test_refusals_before_any_device_work():
    from gcn_grabcut.graph_builder import scissors_list
    from gcn_grabcut.pipeline import _scissors_args
    img = np.zeros((20, 30, 3), np.uint8)
    for anchors in ([(0, 0), (20, 5), (9, 9)], [(0, 0), (5, 30), (9, 9)], [(-1, 0), (5, 5), (9, 9)]):
        with pytest.raises(ValueError, match="outside"):
            trace_boundary(img, anchors)
    with pytest.raises(ValueError):
        trace_boundary(img, [(0, 0), (5, 5)])                             # closed needs three
    with pytest.raises(ValueError):
        trace_boundary(img, [(0, 0)], closed=False)
    with pytest.raises(ValueError):
        trace_boundary(img, [(0, 0), (5, 5), (9, 9)], scissors=(16, 2048, 16))
    assert _scissors_args(None) == Scissors()
    tri = [(0, 0), (0, 5), (5, 0)]
    assert scissors_list(None) == [] and scissors_list(tri) == [tri] and scissors_list([tri, tri[::-1]]) == [tri, tri[::-1]]
    with pytest.raises(ValueError):
        scissors_list("1,2 3,4 5,6")


def test_traced_outlines_join_the_polygons_as_lassos():
    from gcn_grabcut.graph_builder import pack_polygons
    from gcn_grabcut.pipeline import _merge_lassos
    t0, t1 = np.array([(1, 1), (1, 2), (2, 2)], np.int32), np.array([(5, 5), (5, 6), (6, 6), (6, 5)], np.int32)
    tri, quad = [(0, 0), (0, 5), (5, 0)], [(1, 1), (1, 3), (3, 3), (3, 1)]
    assert _merge_lassos(None, [[], [], []]) is None
    polys = pack_polygons([([tri], [quad], []), None, ([], [], [quad])])
    assert _merge_lassos(polys, [[], [], []]) is polys
    only = _merge_lassos(None, [[t0], [], [t1, t0]])
    want = pack_polygons([([], [], [t0]), None, ([], [], [t1, t0])])
    assert all(np.array_equal(x, y) and x.dtype == np.int32 for x, y in zip(only, want))
    verts, pp, pl, ip = _merge_lassos(polys, [[t0], [t1], []])
    assert ip.tolist() == [0, 3, 4, 5] and pl.tolist() == [2, 1, 0, 2, 2] and pp.tolist() == [0, 3, 6, 10, 14, 18]
    assert verts.tolist() == [list(map(int, p)) for p in list(t0) + tri + quad + list(t1) + quad]


# ---------------------------------------------------------------- ABI

def test_header_and_table_carry_the_scissors_entry():
    from gcn_grabcut import _native
    header = (ROOT / "include" / "ggc.h").read_text()
    assert int(re.search(r"#define GGC_VERSION (\d+)", header).group(1)) >= 407
    assert "ggc_trace_paths" in header and "H4" in header
    section = header[header.index("/* H4"):header.index("int ggc_trace_paths")]
    for phrase in ("c(p,q) = L(p,q) * (smooth + F(p) + F(q))", "N, NE, E, SE, S, SW, W, NW", "D(q) + c(p,q) == D(p)", "2^30", "2^29",
                   "64 862", "scissors did not converge", "scissors_planes", "SYNCHRONISES", "1024 * (tiles of the largest window) + 2"):
        assert phrase in section, phrase
    assert len(_native.SIGNATURES["ggc_trace_paths"]) == 17


def test_public_names():
    import gcn_grabcut
    for name in ("pack_paths", "Scissors", "trace_boundary"):
        assert name in gcn_grabcut.__all__ and callable(getattr(gcn_grabcut, name))
    for name in ("segment_scissors", "segment", "segment_batch"):
        assert hasattr(gcn_grabcut.GCNGrabCutPipeline, name)
    import inspect
    assert {"scissors", "scissors_options"} <= set(inspect.signature(gcn_grabcut.GCNGrabCutPipeline.segment).parameters)
    assert "scissors" in inspect.signature(gcn_grabcut.GCNGrabCutPipeline.segment_batch).parameters
    from gcn_grabcut._engine import Engine
    assert hasattr(Engine, "trace_paths") and hasattr(Engine, "upload_paths")


# ---------------------------------------------------------------- CLI

def test_cli_refuses_scissors_on_a_folder_and_bad_options(tmp_path):
    r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--input", str(tmp_path), "--scissors", "3,4 5,6 9,1"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--scissors are anchors on one image" in r.stderr, r.stderr
    r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--image", "x.png", "--scissors", "3,4 5,6 9,1",
                        "--scissors-margin", "300"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "margin" in r.stderr, r.stderr


def test_cli_parses_scissors_flags():
    sys.path.insert(0, str(ROOT))
    import inference
    args = inference.build_parser().parse_args(["--image", "x.png", "--scissors", "100,150 299,399 4,400", "--scissors", "1,2 3,4 5,7",
                                                "--scissors-margin", "8", "--scissors-edge-cap", "900", "--scissors-smooth", "4"])
    assert args.scissors == [[(100, 150), (299, 399), (4, 400)], [(1, 2), (3, 4), (5, 7)]]
    assert (args.scissors_margin, args.scissors_edge_cap, args.scissors_smooth) == (8, 900, 4)
    none = inference.build_parser().parse_args(["--image", "x.png"])
    assert none.scissors == [] and (none.scissors_margin, none.scissors_edge_cap, none.scissors_smooth) == DEFAULTS
    for bad in ("1,2 3,4", "1,2 3,4 5", ""):
        with pytest.raises(SystemExit):
            inference.build_parser().parse_args(["--image", "x.png", "--scissors", bad])
