"""Brush strokes on the host: properties of the stroke rule's restatement (tests/strokes_ref.py), packing per-image strokes
for ggc_apply_strokes, the header / ctypes entries, and the CLI's stroke flags."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import strokes_ref

ROOT = Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------- the rule

def _eight_connected(m):
    """True when the set pixels of m form one 8-connected component."""
    pts = {(int(r), int(c)) for r, c in zip(*np.nonzero(m))}
    if not pts:
        return False
    todo, seen = [next(iter(pts))], set()
    while todo:
        p = todo.pop()
        if p in seen:
            continue
        seen.add(p)
        todo += [(p[0] + dr, p[1] + dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if (p[0] + dr, p[1] + dc) in pts]
    return seen == pts


def test_one_vertex_stroke_is_the_click_disk():
    rng = np.random.default_rng(11)
    for _ in range(60):
        h, w = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        r, c = int(rng.integers(-3, h + 3)), int(rng.integers(-3, w + 3))
        yy, xx = np.mgrid[0:h, 0:w]
        for radius in range(7):
            disk = (yy - r) ** 2 + (xx - c) ** 2 <= radius * radius
            assert np.array_equal(strokes_ref.within(h, w, (r, c, r, c), radius), disk), (h, w, r, c, radius)


def test_centre_line_is_connected_and_holds_both_ends():
    rng = np.random.default_rng(12)
    for _ in range(200):
        h, w = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        a = (int(rng.integers(0, h)), int(rng.integers(0, w)))
        b = (int(rng.integers(0, h)), int(rng.integers(0, w)))
        m = strokes_ref.within(h, w, (*a, *b), 0)
        assert m[a] and m[b], (a, b)
        assert _eight_connected(m), (h, w, a, b)
        extra = int(m.sum()) - (max(abs(a[0] - b[0]), abs(a[1] - b[1])) + 1)
        assert 0 <= extra <= 16, (a, b, extra)


def test_exact_tangency_of_the_3_4_5_segment():
    m = strokes_ref.within(40, 40, (5, 5, 17, 21), 5)
    assert m[15, 10] and not m[16, 10]                 # exactly at distance 5 / just beyond
    assert strokes_ref.within(3, 3, (0, 0, 2, 2), 0).tolist() == \
        [[True, False, False], [False, True, False], [False, False, True]]      # neighbours at distance sqrt(1/2) > 1/2


def _within_signed_64(h, w, seg, radius):
    """The rule with every product in wrapping int64: the shortcut the 128-bit compare exists to avoid."""
    r0, c0, r1, c1 = (np.int64(v) for v in seg[:4])
    rho4 = np.int64(max(4 * radius * radius, 1))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    wy, wx, dy, dx = yy - r0, xx - c0, r1 - r0, c1 - c0
    l2, t, ey, ex, cr = dy * dy + dx * dx, wy * dy + wx * dx, wy - dy, wx - dx, wy * dx - wx * dy
    with np.errstate(over="ignore"):
        mid = np.int64(4) * cr * cr <= rho4 * l2
    return np.where(t <= 0, 4 * (wy * wy + wx * wx) <= rho4, np.where(t >= l2, 4 * (ey * ey + ex * ex) <= rho4, mid))


def test_long_segments_need_more_than_64_bits():
    for i, ((h, w), seg, radius) in enumerate(strokes_ref.LONG_CASES):
        exact = strokes_ref.within(h, w, seg, radius)
        assert exact.any(), i
        if radius == 0:
            assert _eight_connected(exact), i
        if i in strokes_ref.LONG_CASES_BEYOND_64_BITS:
            assert not np.array_equal(_within_signed_64(h, w, seg, radius), exact), i


# ---------------------------------------------------------------- pack_strokes

def test_pack_strokes_order_and_segments():
    from gcn_grabcut.graph_builder import pack_strokes
    strokes, ptr = pack_strokes([([[(1, 2), (3, 4), (5, 6)], [(9, 9)]], [[(7, 8), (7.9, -8.9)]]),
                                 None,
                                 ([], [[(0, 0), (4, 4)]])])
    assert strokes.dtype == np.int32 and ptr.dtype == np.int32
    assert ptr.tolist() == [0, 4, 4, 5]
    assert strokes.tolist() == [[1, 2, 3, 4, 1], [3, 4, 5, 6, 1],        # a polyline of 3 vertices: 2 segments
                                [9, 9, 9, 9, 1],                         # one vertex: both ends equal
                                [7, 8, 7, -8, 0],                        # background after foreground; int(r), int(c)
                                [0, 0, 4, 4, 0]]
    fg, bg = [[(1, 2), (3, 4), (5, 6)], [(9, 9)]], [[(7, 8), (7, -8)]]
    assert strokes[:4].tolist() == [list(s) for s in strokes_ref.segments_of(fg, bg)]


def test_pack_strokes_images_without_strokes_get_empty_ranges():
    from gcn_grabcut.graph_builder import pack_strokes
    strokes, ptr = pack_strokes([None, ((), ()), ([], None), None])
    assert strokes.shape == (0, 5) and ptr.tolist() == [0, 0, 0, 0, 0]
    strokes, ptr = pack_strokes([])
    assert strokes.shape == (0, 5) and ptr.tolist() == [0]


def test_pack_strokes_keeps_vertices_outside_the_image():
    from gcn_grabcut.graph_builder import pack_strokes
    strokes, ptr = pack_strokes([([[(-30000, -30000), (30020, 30030)]], [[(2**20, -2**20)]])])
    assert strokes.tolist() == [[-30000, -30000, 30020, 30030, 1], [2**20, -2**20, 2**20, -2**20, 0]]
    assert ptr.tolist() == [0, 2]


@pytest.mark.parametrize("bad", [
    [([[]], [])],                          # an empty stroke
    [([[(1, 2, 3)]], [])],                 # three coordinates
    [([(1, 2), (3, 4)], [])],              # a stroke's vertices given where the list of strokes belongs
    [([[(1, 2)]],)],                       # an entry that is not a (fg, bg) pair
    ["ab"],
    [(["ab"], [])],
    [([[(float("nan"), 2)]], [])],
    [([[(2**20 + 1, 0)]], [])],            # beyond the kernel's coordinate limit
])
def test_pack_strokes_rejects_bad_shapes(bad):
    from gcn_grabcut.graph_builder import pack_strokes
    with pytest.raises(ValueError):
        pack_strokes(bad)


# ---------------------------------------------------------------- ABI

def test_header_and_table_carry_the_stroke_entries():
    from gcn_grabcut import _native
    header = (ROOT / "include" / "ggc.h").read_text()
    assert int(re.search(r"#define GGC_VERSION (\d+)", header).group(1)) >= 405
    assert "ggc_apply_strokes" in header and "ggc_stroke_pixels" in header
    assert len(_native.SIGNATURES["ggc_apply_strokes"]) == 9
    assert len(_native.SIGNATURES["ggc_stroke_pixels"]) == 10


def test_public_names():
    import gcn_grabcut
    for name in ("pack_strokes", "paint_strokes", "stroke_pixels"):
        assert name in gcn_grabcut.__all__ and callable(getattr(gcn_grabcut, name))
    assert hasattr(gcn_grabcut.GrabCut, "add_strokes")


def test_stroke_arguments_are_checked_before_the_device():
    from gcn_grabcut.pipeline import _Hints
    assert _Hints.of(None, 3, 5, False, False, None, None) is None
    assert _Hints.of(None, 3, 5, False, False, None, [None, None, None]) is None
    assert _Hints.of(None, 3, 5, False, False, None, [None, ([], []), None]) is None
    h = _Hints.of(None, 3, 5, False, False, None, [None, ([[(1, 1), (2, 5)]], []), ([], [[(0, 0)]])], 4)
    assert h.rows.shape == (0, 3) and h.ptr.tolist() == [0, 0, 0, 0]
    assert h.seg_ptr.tolist() == [0, 0, 1, 2] and h.stroke_radius == 4
    assert h.chunk(0, 1) is None                                        # neither clicks nor strokes in the chunk
    c = h.chunk(1, 3)
    assert c.seg_ptr.tolist() == [0, 1, 2] and c.segs.tolist() == h.segs.tolist()
    c = h.chunk(2, 3)
    assert c.seg_ptr.tolist() == [0, 1] and c.segs.tolist() == [[0, 0, 0, 0, 0]]
    only_clicks = _Hints.of([None, ([(1, 1)], []), None], 3, 5, False, False)
    assert only_clicks.segs is None and only_clicks.chunk(0, 3).segs is None
    with pytest.raises(ValueError):
        _Hints.of(None, 3, 5, False, False, None, [None, None])         # wrong length
    for bad in (-1, 16385, 2.5):
        with pytest.raises(ValueError):
            _Hints.of(None, 1, 5, False, False, None, [([[(1, 1)]], [])], bad)


# ---------------------------------------------------------------- CLI

def test_cli_refuses_strokes_on_a_folder(tmp_path):
    for flag in ("--fg-stroke", "--bg-stroke"):
        r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--input", str(tmp_path), flag, "3,4 5,6"],
                           cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0
        assert "--image" in r.stderr


def test_cli_parses_and_scales_stroke_vertices():
    sys.path.insert(0, str(ROOT))
    import inference
    args = inference.build_parser().parse_args(["--image", "x.png", "--bg-stroke", "100,150 299,399 -4,400",
                                                "--bg-stroke", "7,8", "--fg-stroke", "1,2 3,4", "--stroke-radius", "2"])
    assert args.bg_stroke == [[(100, 150), (299, 399), (-4, 400)], [(7, 8)]]
    assert args.fg_stroke == [[(1, 2), (3, 4)]] and args.stroke_radius == 2
    assert [inference.scale_points(s, (300, 400), (150, 200)) for s in args.bg_stroke] == \
        [[(50, 75), (149, 199), (-2, 200)], [(3, 4)]]
    with pytest.raises(SystemExit):
        inference.build_parser().parse_args(["--image", "x.png", "--bg-stroke", "1,2 3"])
