"""Mask outlines without a device: the definition of include/ggc.h K1 as tests/outlines_ref.py restates it, on masks small
enough to check by hand and on random ones through the properties the header promises; then the Python layer around
ggc_mask_outlines (Outline, the two helpers, refusals, the export, the command line's parsing)."""
import re
from pathlib import Path

import numpy as np
import pytest
from scipy import ndimage

import outlines_ref as ref
import polygons_ref

ROOT = Path(__file__).resolve().parent.parent


def loops_of(mask, connectivity=8):
    return [(lp["vertices"], lp["area"], lp["outer"], lp["perimeter"]) for lp in ref.trace(np.array(mask, np.uint8), connectivity)]


# ---- by hand -------------------------------------------------------------------------------------------------------
def test_one_pixel():
    assert loops_of([[1]]) == [([(0, 0), (0, 1), (1, 1), (1, 0)], 1, 0, 4)]
    assert loops_of([[7]], 4) == [([(0, 0), (0, 1), (1, 1), (1, 0)], 1, 0, 4)]          # any nonzero byte
    assert loops_of([[0]]) == [] and loops_of([[0]], 4) == []


def test_full_image():
    for conn in (4, 8):
        assert loops_of(np.ones((2, 3)), conn) == [([(0, 0), (0, 3), (2, 3), (2, 0)], 6, 0, 10)]


def test_two_diagonal_pixels():
    m = [[1, 0], [0, 1]]
    assert loops_of(m, 8) == [([(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 1), (1, 1), (1, 0)], 2, 0, 8)]
    assert loops_of(m, 4) == [([(0, 0), (0, 1), (1, 1), (1, 0)], 1, 0, 4), ([(1, 1), (1, 2), (2, 2), (2, 1)], 1, 1, 4)]
    m = [[0, 1], [1, 0]]
    assert loops_of(m, 8) == [([(0, 1), (0, 2), (1, 2), (1, 1), (2, 1), (2, 0), (1, 0), (1, 1)], 2, 0, 8)]
    assert loops_of(m, 4) == [([(0, 1), (0, 2), (1, 2), (1, 1)], 1, 0, 4), ([(1, 0), (1, 1), (2, 1), (2, 0)], 1, 1, 4)]


def test_ring():
    ring = np.ones((3, 3), np.uint8)
    ring[1, 1] = 0
    for conn in (4, 8):
        got = ref.trace(ring, conn)
        assert loops_of(ring, conn) == [([(0, 0), (0, 3), (3, 3), (3, 0)], 9, 0, 12), ([(1, 1), (2, 1), (2, 2), (1, 2)], -1, 0, 4)]
        assert got[1]["start"] == (1, 1, 1)                    # the hole starts at (1, 1) going S
        ref.check_properties(ring, got, conn, polygons_ref.covered)


def test_ring_with_an_island_in_its_hole():
    m = np.ones((5, 5), np.uint8)
    m[1:4, 1:4] = 0
    m[2, 2] = 1
    for conn in (4, 8):
        assert loops_of(m, conn) == [([(0, 0), (0, 5), (5, 5), (5, 0)], 25, 0, 20), ([(1, 1), (4, 1), (4, 4), (1, 4)], -9, 0, 12),
                                     ([(2, 2), (2, 3), (3, 3), (3, 2)], 1, 2, 4)]
        ref.check_properties(m, ref.trace(m, conn), conn, polygons_ref.covered)


def test_hole_that_touches_the_outer_loop_at_a_saddle():
    m = np.array([[1, 1, 1], [1, 0, 1], [1, 1, 0]], np.uint8)
    assert loops_of(m, 8) == [([(0, 0), (0, 3), (2, 3), (2, 2), (3, 2), (3, 0)], 8, 0, 12), ([(1, 1), (2, 1), (2, 2), (1, 2)], -1, 0, 4)]
    assert loops_of(m, 4) == [([(0, 0), (0, 3), (2, 3), (2, 2), (1, 2), (1, 1), (2, 1), (2, 2), (3, 2), (3, 0)], 7, 0, 16)]


# ---- the properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.3, 0.5, 0.7])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_properties_on_random_masks(density, connectivity):
    rng = np.random.default_rng(int(density * 10) * 16 + connectivity)
    for _ in range(12):
        h, w = int(rng.integers(1, 13)), int(rng.integers(1, 15))
        m = (rng.random((h, w)) < density).astype(np.uint8) * int(rng.choice([1, 255]))
        loops = ref.trace(m, connectivity)
        ref.check_properties(m, loops, connectivity, polygons_ref.covered_np)
        full = np.ones((3, 3), int)
        cross = ndimage.generate_binary_structure(2, 1)
        assert sum(lp["area"] > 0 for lp in loops) == ndimage.label(m, full if connectivity == 8 else cross)[1]
        bg = np.pad(m == 0, 1, constant_values=True)
        assert sum(lp["area"] < 0 for lp in loops) == ndimage.label(bg, cross if connectivity == 8 else full)[1] - 1


def test_round_trip_by_the_plain_point_rule():
    rng = np.random.default_rng(5)
    for conn in (4, 8):
        m = (rng.random((5, 6)) < 0.5).astype(np.uint8)
        assert np.array_equal(ref.fill_back(m.shape, ref.trace(m, conn), polygons_ref.covered), m != 0)


def test_transposing_the_mask_mirrors_every_loop():
    rng = np.random.default_rng(11)
    for conn in (4, 8):
        for _ in range(10):
            m = (rng.random((int(rng.integers(1, 11)), int(rng.integers(1, 11)))) < 0.5).astype(np.uint8)
            a, b = ref.trace(m, conn), ref.trace(m.T.copy(), conn)
            assert sorted((lp["area"], lp["perimeter"]) for lp in a) == sorted((lp["area"], lp["perimeter"]) for lp in b)
            # the mirrored loop runs the other way round: the same corners, transposed
            assert sorted(sorted(lp["vertices"]) for lp in a) == sorted(sorted((c, r) for r, c in lp["vertices"]) for lp in b)


@pytest.mark.parametrize("shape", [(1, 1), (3, 4), (4, 4), (5, 7)])
def test_the_checkerboard_against_the_crack_bound(shape):
    """2HW + H + W is the number of unit edges of the image, each a crack at most once.  On the checkerboard every edge
    between two pixels is a crack and every set pixel has all four of its edges; what is missing to the bound are the
    border edges of the clear pixels, so only the 1 x 1 board reaches it exactly."""
    h, w = shape
    bound = 2 * h * w + h + w
    board = (np.add.outer(np.arange(h), np.arange(w)) % 2 == 0).astype(np.uint8)
    other = 1 - board
    border_clear = int((board[0] == 0).sum() + (board[-1] == 0).sum() + (board[:, 0] == 0).sum() + (board[:, -1] == 0).sum())
    assert len(ref.cracks(board)) == 4 * int(board.sum()) == bound - border_clear
    assert len(ref.cracks(board)) + len(ref.cracks(other)) == 2 * bound - (2 * h + 2 * w)      # the frame's edges count once
    if shape == (1, 1):
        assert len(ref.cracks(board)) == bound
    rng = np.random.default_rng(0)
    for _ in range(8):
        assert len(ref.cracks((rng.random(shape) < 0.5).astype(np.uint8))) <= len(ref.cracks(board)) <= bound


def test_pack_is_the_polygon_packing():
    per_image = [ref.trace(np.array(m, np.uint8)) for m in ([[1, 0], [0, 0]], [[0, 0], [0, 0]], [[1, 1, 1], [1, 0, 1], [1, 1, 1]])]
    verts, loop_ptr, info, image_ptr, image_vert_ptr = ref.pack(per_image)
    assert image_ptr.tolist() == [0, 1, 1, 3] and image_vert_ptr.tolist() == [0, 4, 4, 12] and loop_ptr.tolist() == [0, 4, 8, 12]
    assert info.tolist() == [[1, 0, 4], [9, 0, 12], [-1, 0, 4]] and verts.shape == (12, 2) and verts.dtype == np.int32


# ---- the Python layer ---------------------------------------------------------------------------------------------------
def test_outline_and_helpers():
    import gcn_grabcut as g
    from dataclasses import FrozenInstanceError
    outer = g.Outline(np.array([(0, 0), (0, 3), (3, 3), (3, 0)], np.int32), 9, 12, 0)
    hole = g.Outline(np.array([(1, 1), (2, 1), (2, 2), (1, 2)], np.int32), -1, 4, 0)
    assert not outer.hole and hole.hole
    with pytest.raises(FrozenInstanceError):
        outer.area = 3
    assert g.outlines_svg_path([outer, hole]) == "M 0 0 L 3 0 L 3 3 L 0 3 Z M 1 1 L 1 2 L 2 2 L 2 1 Z"
    assert g.outlines_svg_path([]) == ""
    lassos = g.outlines_to_lassos([outer, hole])
    assert len(lassos) == 1 and lassos[0].tolist() == outer.vertices.tolist() and lassos[0] is not outer.vertices
    for name in ("Outline", "mask_outlines", "mask_outlines_batch", "outlines_svg_path", "outlines_to_lassos"):
        assert name in g.__all__ and hasattr(g, name)


def test_python_layer_refuses_before_any_device_work():
    import gcn_grabcut as g
    with pytest.raises(ValueError, match="must be \\(H, W\\)"):
        g.mask_outlines(np.zeros((2, 3, 4), np.uint8))
    with pytest.raises(ValueError, match="must be \\(H, W\\)"):
        g.mask_outlines(np.zeros(5, np.uint8))
    with pytest.raises(ValueError, match="must be \\(B, H, W\\)"):
        g.mask_outlines_batch(np.zeros((2, 3), np.uint8))
    for bad in (0, 6, "8", None):
        with pytest.raises(ValueError, match="connectivity"):
            g.mask_outlines(np.zeros((2, 3), np.uint8), connectivity=bad)
    with pytest.raises(ValueError, match="empty masks"):
        g.mask_outlines_batch(np.zeros((2, 0, 3), np.uint8))
    assert g.mask_outlines_batch(np.zeros((0, 4, 4), np.uint8)) == []


def test_result_without_full_outputs_refuses_full_outlines():
    from gcn_grabcut import SegmentationResult
    import dataclasses
    z = np.zeros((2, 2), np.uint8)
    r = SegmentationResult(image=np.zeros((2, 2, 3), np.uint8), binary_mask=z, trimap=z, segments=z.astype(np.int32),
                           overlay=np.zeros((2, 2, 3), np.uint8), rgba=np.zeros((2, 2, 4), np.uint8))
    with pytest.raises(ValueError, match="full"):
        r.outlines(full=True)
    with pytest.raises(ValueError, match="connectivity"):
        r.outlines(connectivity=6)
    assert "outlines" not in {f.name for f in dataclasses.fields(SegmentationResult)}      # a method, not a field


def test_header_section_and_signature():
    from gcn_grabcut import _native
    header = (ROOT / "include" / "ggc.h").read_text()
    section = header[header.index("/* K1"):header.index("int ggc_mask_outlines")]
    for phrase in ("CORNER LATTICE", "CRACKS", "SUCCESSOR", "LOOPS", "smallest key", "SYNCHRONISES", "Scratch", "image groups",
                   "left (d+3)&3, straight d, right (d+1)&3", "2HW + H + W", "GGC_E_SHAPE", "GGC_E_INVALID_ARG"):
        assert phrase in section, phrase
    assert header.index("/* K0") < header.index("/* K1") < header.index("/* O0")
    assert len(_native.SIGNATURES["ggc_mask_outlines"]) == 14
    assert int(re.search(r"#define GGC_VERSION (\d+)", header).group(1)) >= 408


def test_command_line_parses_the_outline_options():
    import inference
    p = inference.build_parser()
    a = p.parse_args(["--image", "x.png", "--save", "mask", "outlines"])
    assert "outlines" in a.save and a.outline_connectivity == 8
    assert p.parse_args(["--image", "x.png", "--outline-connectivity", "4"]).outline_connectivity == 4
    with pytest.raises(SystemExit):
        p.parse_args(["--image", "x.png", "--outline-connectivity", "6"])


def test_outlines_document():
    import inference
    import json
    from gcn_grabcut import Outline
    loops = [Outline(np.array([(0, 0), (0, 3), (2, 3), (2, 0)], np.int32), 6, 10, 0)]
    doc = json.loads(json.dumps(inference.outlines_document((2, 3), loops, 8)))
    assert doc == {"height": 2, "width": 3, "connectivity": 8, "svg_path": "M 0 0 L 3 0 L 3 2 L 0 2 Z",
                   "loops": [{"vertices": [[0, 0], [0, 3], [2, 3], [2, 0]], "area": 6, "perimeter": 10, "outer": 0}]}
