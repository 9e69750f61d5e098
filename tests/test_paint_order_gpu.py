"""The order-keeping list of the tile painter ("The tile painter") on the MI355X, for clicks, strokes and polygons.

One 16 x 96 image (3 x 2 tiles of 32 x 8) and an empty second one.  The labels alternate with the index and the primitives
overlap, so the label of a pixel says which index won there.  Two of three primitives lie in the left tile and the third in
the right-hand one: every wave of 64 candidates of a tile keeps some and drops some, so a keeper's slot in the list differs
from its index and depends on the other waves' counts; the counts 255, 256, 257 and 513 end a pass just below, at and just
above the list's 256 entries.  The packed arrays are built here, not by pack_*; the expectation is the restatement of each
rule (tests/strokes_ref.py, tests/polygons_ref.py, a numpy loop for the disks) applied in index order."""
import numpy as np
import pytest

import polygons_ref
import strokes_ref

pytestmark = pytest.mark.gpu
H, W = 16, 96
RADIUS = 2
POISON = 7


@pytest.fixture(scope="module")
def eng():
    from gcn_grabcut._engine import get_engine
    return get_engine("cuda")


def _masks():
    return np.full((2, H, W), POISON, np.uint8)        # poison: an untouched pixel is neither read nor written


def _check(got, want):
    assert np.array_equal(got, want)
    assert (got[1] == POISON).all()                     # the empty image
    assert (got[0, :, 32:64] == POISON).all()           # the middle tiles: nothing reaches them
    for part in (got[0, :, :32], got[0, :, 64:]):       # both labels and untouched pixels on either side
        assert (part == 0).any() and (part == 1).any() and (part == POISON).any()


def _place(k):
    """Primitive k's anchor (row, col): four anchors of a 2 x 2 patch in the left tile, every third one in the right tile."""
    return 3 + (k // 2) % 2, (80 if k % 3 == 2 else 10) + (k // 4) % 2


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_clicks_are_painted_in_index_order(eng, n):
    rows = np.array([(*_place(k), k % 2) for k in range(n)], np.int32)
    ptr = np.array([0, n, n], np.int32)
    masks = _masks()
    d_rows, d_ptr = eng.upload_hints(rows, ptr)
    got = eng.apply_hints(eng.to_device(masks), d_rows, d_ptr, RADIUS).cpu().numpy()
    want = masks.copy()
    yy, xx = np.mgrid[0:H, 0:W]
    for r, c, l in rows:                                # the disk rule, later clicks over earlier ones
        want[0][(yy - r) ** 2 + (xx - c) ** 2 <= RADIUS * RADIUS] = l
    _check(got, want)
    # the same list as one-point segments through the strokes' restatement
    assert np.array_equal(want[0], strokes_ref.paint(masks[0], [(r, c, r, c, l) for r, c, l in rows], RADIUS))


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_segments_are_painted_in_index_order(eng, n):
    segs = []
    for k in range(n):
        r, c = _place(k)
        segs.append((r, c - 2, r + 1 - 2 * (k % 2), c + 3, k % 2))     # short and slanted either way
    strokes, ptr = np.array(segs, np.int32), np.array([0, n, n], np.int32)
    masks = _masks()
    d_strokes, d_ptr = eng.upload_strokes(strokes, ptr)
    got = eng.apply_strokes(eng.to_device(masks), d_strokes, d_ptr, RADIUS).cpu().numpy()
    want = masks.copy()
    want[0] = strokes_ref.paint(masks[0], segs, RADIUS)
    _check(got, want)


@pytest.mark.parametrize("n", [85, 86, 171])
def test_polygon_edges_are_painted_in_index_order(eng, n):
    """Triangles: 255, 258 and 513 edges, so a polygon straddles the end of a pass.  They reach from the upper tile into
    the lower one, whose row test drops one or two edges of each."""
    verts = []
    for k in range(n):
        r, c = _place(k)
        verts += [(r - 2, c - 3), (r - 1 + k % 2, c + 5), (r + 5 + (k // 2) % 3, c)]
    packed = (np.array(verts, np.int32), 3 * np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32) % 2,
              np.array([0, n, n], np.int32))
    masks = _masks()
    got = eng.apply_polygons(eng.to_device(masks), *eng.upload_polygons(*packed)).cpu().numpy()
    _check(got, polygons_ref.apply_packed(masks, *packed))
