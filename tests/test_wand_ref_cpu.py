"""tests/wand_ref.py, the reference of the magic wand, held to cases worked out by hand.  No device is needed."""
import numpy as np

import wand_ref as ref


def grey(plane):
    return np.ascontiguousarray(np.repeat(np.asarray(plane, np.uint8)[:, :, None], 3, axis=2))


def test_a_diagonal_is_one_component_with_8_neighbours_only():
    img = grey(np.where(np.eye(5, dtype=bool), 200, 10))
    assert ref.selection(img, 0, 0, 0, 4, 1).astype(int).tolist() == [[1, 0, 0, 0, 0]] + [[0] * 5] * 4
    assert np.array_equal(ref.selection(img, 0, 0, 0, 8, 1), np.eye(5, dtype=bool))
    assert np.array_equal(ref.selection(img, 2, 2, 0, 0, 1), np.eye(5, dtype=bool))             # not contiguous: all of them
    off = ref.selection(img, 0, 1, 0, 4, 1)                    # the upper triangle of the background; the lower is cut off
    assert off.sum() == 10 and off[0, 4] and not off[4, 0]
    assert ref.selection(img, 0, 1, 0, 0, 1).sum() == 20


def test_tolerance_0_and_255():
    img = grey([[10, 11, 10], [12, 10, 9]])
    assert ref.selection(img, 0, 0, 0, 8, 1).astype(int).tolist() == [[1, 0, 1], [0, 1, 0]]
    assert ref.selection(img, 0, 0, 0, 4, 1).astype(int).tolist() == [[1, 0, 0], [0, 0, 0]]
    assert ref.selection(img, 0, 0, 1, 4, 1).astype(int).tolist() == [[1, 1, 1], [0, 1, 1]]
    assert ref.selection(img, 0, 0, 255, 4, 1).all()
    wild = np.array([[[0, 255, 0], [255, 0, 255]]], np.uint8)
    assert ref.selection(wild, 0, 0, 255, 4, 1).all() and ref.selection(wild, 0, 0, 254, 4, 1).sum() == 1
    one_channel = np.array([[[10, 10, 10], [10, 10, 30]]], np.uint8)                           # the max-channel metric
    assert ref.selection(one_channel, 0, 0, 19, 4, 1).sum() == 1 and ref.selection(one_channel, 0, 0, 20, 4, 1).sum() == 2


def test_sample_3_at_a_corner_replicates_the_border():
    b = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]])
    img = np.stack([b, 2 * b, np.zeros_like(b)], axis=2).astype(np.uint8)
    # rows -1, 0, 1 -> 0, 0, 1 and columns -1, 0, 1 -> 0, 0, 1: (10 + 10 + 20) twice, then 40 + 40 + 50
    assert ref.ref_sums(img, 0, 0, 3) == [40 + 40 + 130, 2 * (40 + 40 + 130), 0]
    # the far corner: rows 1, 2, 2 and columns 1, 2, 2: 50 + 60 + 60, then (80 + 90 + 90) twice
    assert ref.ref_sums(img, 2, 2, 3) == [170 + 260 + 260, 2 * (170 + 260 + 260), 0]
    assert ref.ref_sums(img, 1, 1, 3) == [450, 900, 0] and ref.ref_sums(img, 1, 1, 1) == [50, 100, 0]
    assert ref.ref_sums(img, 1, 1, 5) == [sum(b[min(max(y, 0), 2), min(max(x, 0), 2)] for y in range(-1, 4) for x in range(-1, 4)),
                                         2 * sum(b[min(max(y, 0), 2), min(max(x, 0), 2)] for y in range(-1, 4) for x in range(-1, 4)), 0]
    # match against the sum 210 of the corner: 9 * 10 = 90 is 120 away, 9 * 20 = 180 is 30 away (channel 1 doubles both)
    assert not ref.match_one(img[0, 0], [210, 420, 0], 13, 3) and ref.match_one(img[0, 0], [210, 420, 0], 27, 3)
    assert ref.match_one(img[0, 1], [210, 420, 0], 7, 3) and not ref.match_one(img[0, 1], [210, 420, 0], 6, 3)


def test_a_seed_that_fails_its_own_averaged_reference_selects_nothing():
    plane = np.full((5, 5), 100)
    plane[2, 2] = 0                                           # the seed: 9 * 0 against 800 is off by 800 > 9 * 50
    img = grey(plane)
    assert ref.ref_sums(img, 2, 2, 3) == [800, 800, 800]
    for conn in (4, 8):
        assert not ref.selection(img, 2, 2, 50, conn, 3).any()
    assert ref.selection(img, 2, 2, 50, 0, 3).sum() == 24     # not contiguous: the ring around it still matches
    mask, select, counts = ref.wand_image(img, [(2, 2, 1)], 50, 8, 3, np.full((5, 5), 2, np.uint8))
    assert (mask == 2).all() and not select.any() and counts.tolist() == [0, 0]


def test_order_decides_where_selections_overlap():
    plane = np.zeros((2, 6), int)
    plane[:, 3:] = 20
    img = grey(plane)
    start = np.array([[0, 1, 2, 3, 0, 1], [2, 3, 0, 1, 2, 3]], np.uint8)
    # foreground takes everything (tolerance 20), then background the right half (tolerance 0 would; here its own half at 20 is all)
    m, s, c = ref.wand_image(img, [(0, 0, 1), (0, 5, 0)], 20, 4, 1, start)
    assert (m == 0).all() and not s.any() and c.tolist() == [0, 12]
    m, s, c = ref.wand_image(img, [(0, 5, 0), (0, 0, 1)], 20, 4, 1, start)
    assert (m == 1).all() and (s == 255).all() and c.tolist() == [12, 0]
    m, s, c = ref.wand_image(img, [(0, 0, 1), (0, 5, 0)], 0, 4, 1, start)            # disjoint halves
    assert m.tolist() == [[1, 1, 1, 0, 0, 0]] * 2 and s.tolist() == [[255, 255, 255, 0, 0, 0]] * 2 and c.tolist() == [6, 6]
    m, s, c = ref.wand_image(img, [(0, 0, 1)], 0, 4, 1, start)                       # undecided pixels keep their label
    assert m[:, 3:].tolist() == start[:, 3:].tolist() and c.tolist() == [6, 0]


def test_a_seed_outside_the_image_is_ignored():
    img = grey(np.zeros((3, 4), int))
    for seed in ((-1, 0, 1), (0, -1, 1), (3, 0, 1), (0, 4, 1)):
        m, s, c = ref.wand_image(img, [seed], 0, 8, 1, np.full((3, 4), 3, np.uint8))
        assert (m == 3).all() and not s.any() and c.tolist() == [0, 0]
    m, s, c = ref.wand_image(img, [(3, 0, 0), (1, 1, 1)], 0, 8, 1)
    assert m is None and (s == 255).all() and c.tolist() == [12, 0]
    m, s, c = ref.wand_batch(np.stack([img, img]), [(0, 0, 1), (9, 9, 0)], [0, 1, 2], 0, 8, 1, np.full((2, 3, 4), 2, np.uint8))
    assert (m[0] == 1).all() and (m[1] == 2).all() and c.tolist() == [[12, 0], [0, 0]]
