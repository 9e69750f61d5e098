"""The label-map builders of graph_cases.py hold the properties that the on-chip limit tests rest on: exact pair counts
around the table's 6144 entries, which of eight row bands overflows, the region counts around 704, and how many of the
fuzz's 40 batches fit the tables.  Pairs are counted here a second time, pixel link by pixel link into a Python set, so
that graph_cases.pair_keys (which the builders and the predictions use) and the maps cannot drift off the limits together."""
import numpy as np
import pytest

import graph_cases as gc
from test_graph_onchip_gpu import CASES


def pair_set(seg, conn, y0=0, y1=None):
    """{(min, max)} over the right and down links of the rows [y0, y1), and both diagonals at connectivity 8."""
    h, w = seg.shape
    y1 = h if y1 is None else min(y1, h)
    out = set()

    def link(u, v):
        if u != v:
            out.add((min(u, v), max(u, v)))
    s = seg.tolist()
    for y in range(y0, y1):
        for x in range(w):
            if x + 1 < w:
                link(s[y][x], s[y][x + 1])
            if y + 1 < h:
                link(s[y][x], s[y + 1][x])
            if conn == 8 and x + 1 < w and y + 1 < h:
                link(s[y][x], s[y + 1][x + 1])
                link(s[y][x + 1], s[y + 1][x])
    return out


def band_sets(seg, conn, bands):
    h = seg.shape[0]
    rows_per = (h + bands - 1) // bands                   # k_region_scan's split
    return [pair_set(seg, conn, min(g * rows_per, h), min((g + 1) * rows_per, h)) for g in range(bands)]


def all_labels_occur(seg):
    return seg.dtype == np.int32 and np.array_equal(np.unique(seg), np.arange(int(seg.max()) + 1))


@pytest.mark.parametrize("seg,conn", [(gc.hub(), 4), (gc.hub(), 8), (gc.blocks(9, 70, 2, 8), 8), (gc.stripes(3, 70, False), 8),
                                      (gc.blocks(1, 200, 1, 8), 8), (gc.stripes(5, 1, False), 8),
                                      (gc.scattered(20, 30, 50, 1), 4), (gc.scattered(20, 30, 50, 1), 8)])
def test_the_numpy_counter_agrees_with_the_set_of_links(seg, conn):
    n = int(seg.max()) + 1
    assert sorted(lo * n + hi for lo, hi in pair_set(seg, conn)) == list(gc.pair_keys(seg, conn))
    for bands in (1, 2, 3, 5, 8):
        want = [len(s) for s in band_sets(seg, conn, min(bands, seg.shape[0]))]
        assert gc.band_pair_counts(seg, conn, bands) == want


@pytest.mark.parametrize("target", [6143, 6144, 6145])
def test_exact_pairs_has_exactly_the_target(target):
    seg = gc.exact_pairs(target)
    assert seg.shape == (128, 96) and all_labels_occur(seg) and int(seg.max()) + 1 <= gc.NODE_LIMIT
    assert len(pair_set(seg, 4)) == target == gc.pair_count(seg, 4)
    assert max(len(s) for s in band_sets(seg, 4, 8)) < gc.PAIR_LIMIT       # at 8 bands only the union can overflow


def test_euler_circuit_uses_every_pair_once():
    walk = gc.euler_circuit(113)
    steps = {(min(a, b), max(a, b)) for a, b in zip(walk, walk[1:])}
    assert len(walk) == 113 * 112 // 2 + 1 and len(steps) == 113 * 112 // 2 and walk[0] == walk[-1]


def test_one_band_overflow_fills_the_first_of_eight_bands_only():
    seg = gc.one_band_overflow()
    assert seg.shape == (256, 96) and all_labels_occur(seg) and int(seg.max()) + 1 == gc.NODE_LIMIT
    counts = [len(s) for s in band_sets(seg, 8, 8)]
    assert counts[0] > gc.PAIR_LIMIT and all(c < gc.PAIR_LIMIT for c in counts[1:])
    assert counts == gc.band_pair_counts(seg, 8, 8)


def test_too_many_pairs_overflows_in_the_union_not_in_a_band():
    """At eight bands no band's table fills: the case is the union overflow of k_topology.  (With one band, as the
    benchmark's batch runs, the scan's own insert overflows; exact_pairs(6145) and one_band_overflow are for that.)"""
    make, conn, _, _ = CASES["too_many_pairs"]
    seg = make()[0]
    assert all(len(s) <= gc.PAIR_LIMIT for s in band_sets(seg, conn, 8))
    assert len(pair_set(seg, conn)) > gc.PAIR_LIMIT
    assert gc.band_pair_counts(seg, conn, 1)[0] == gc.pair_count(seg, conn) == len(pair_set(seg, conn))


@pytest.mark.parametrize("h,w,n,seed", [(48, 64, 60, 1), (48, 64, 60, 4), (1, 50, 7, 0), (33, 1, 9, 2), (5, 5, 25, 3), (20, 20, 1, 0)])
def test_voronoi_labels_are_nearest_sites_and_all_occur(h, w, n, seed):
    seg = gc.voronoi(h, w, n, seed)
    assert seg.shape == (h, w) and all_labels_occur(seg) and int(seg.max()) + 1 <= n
    assert np.array_equal(seg, gc.voronoi(h, w, n, seed))
    rng = np.random.default_rng(seed)
    sy, sx = rng.integers(0, h, n), rng.integers(0, w, n)
    for y, x in [(0, 0), (h - 1, w - 1), (h // 2, w // 3)]:
        d2 = (sy - y) ** 2 + (sx - x) ** 2
        same = seg == seg[y, x]
        assert same[sy[np.argmin(d2)], sx[np.argmin(d2)]]            # the pixel shares its label with its nearest site


def test_voronoi_regions_are_irregular():
    seg = gc.voronoi(48, 64, 60, 1)
    n = int(seg.max()) + 1
    degree = np.bincount(np.array(sorted(pair_set(seg, 8))).ravel(), minlength=n)
    area = np.bincount(seg.ravel())
    assert degree.max() >= 2 * degree.min() and area.max() >= 8 * area.min()


@pytest.mark.parametrize("n", [703, 704, 705])
def test_region_limit_has_n_regions(n):
    seg = gc.region_limit(n)
    assert seg.shape == (44, 64) and all_labels_occur(seg) and int(seg.max()) + 1 == n
    assert gc.pair_count(seg, 8) < gc.PAIR_LIMIT


def test_limit_cases_take_the_paths_they_name():
    for name, (make, conn, k, _, path) in gc.LIMIT_CASES.items():
        segs = make()
        assert all(all_labels_occur(s) for s in segs) and len({s.shape for s in segs}) == 1, name
        assert gc.predict(segs, conn, k) == path, name
    want = {"too_many_nodes": "dense", "too_many_pairs": "overflow"}
    for name, (make, conn, k, _) in CASES.items():
        assert gc.predict(make(), conn, k) == want.get(name, "onchip"), name


def test_limit_cases_stand_at_the_limits():
    n_of = {name: [int(s.max()) + 1 for s in c[0]()] for name, c in gc.LIMIT_CASES.items()}
    assert n_of["ragged704"] == [704, 1, 5] and n_of["n10_k8"] == [10] and n_of["n9_k8"] == [9]
    assert gc.LIMIT_CASES["voronoi_k5"][2] == 5 and gc.LIMIT_CASES["voronoi_k0"][2] == 0
    assert gc.LIMIT_CASES["rows9"][0]()[0].shape[0] == 9 and gc.LIMIT_CASES["rows3"][0]()[0].shape[0] == 3
    assert gc.LIMIT_CASES["rows1"][0]()[0].shape[0] == 1
    lab = gc.flat_lab(np.random.default_rng(0).random((1, 4, 5, 3)).astype(np.float32))
    assert len(np.unique(lab.reshape(-1, 3), axis=0)) == 1


@pytest.fixture(scope="module")
def fuzz(oracle):
    """Every fuzz case with its maps (SLIC by the oracle here) and predicted path."""
    def slic(bgr, n_seg):
        return [oracle.slic(oracle.preprocess(im)[0], n_seg)[0] for im in bgr]
    out = []
    for i in range(gc.FUZZ_COUNT):
        case = gc.fuzz_case(i)
        segs = gc.fuzz_maps(case, slic)
        out.append((case, segs, gc.predict(segs, case["conn"], case["k"])))
    return out


def test_fuzz_seed_puts_at_least_30_of_40_cases_on_chip(fuzz):
    paths = [p for _, _, p in fuzz]
    assert len(paths) == 40 and paths.count("onchip") >= 30
    for part in range(gc.FUZZ_PARTS):                     # each child process of the GPU test holds its share
        third = paths[part::gc.FUZZ_PARTS]
        assert third.count("onchip") >= 10 and third.count("overflow") >= 1, part
    assert paths.count("dense") >= 1


def test_fuzz_cases_span_what_the_issue_asks(fuzz):
    cases = [c for c, _, _ in fuzz]
    assert (cases[0]["h"], cases[1]["w"]) == (1, 1)
    assert all(1 <= c["h"] <= 130 and 1 <= c["w"] <= 130 and 1 <= c["b"] <= 6 for c in cases)
    assert {c["kind"] for c in cases} == set(gc.FUZZ_KINDS) and {c["conn"] for c in cases} == {4, 8}
    assert {c["k"] for c in cases} == set(range(9)) and {c["b"] for c in cases} == set(range(1, 7))
    for case, segs, _ in fuzz:
        assert len(segs) == case["b"] and all(s.shape == (case["h"], case["w"]) and all_labels_occur(s) for s in segs), case
    scattered = [max(gc.pair_count(s, c["conn"]) for s in segs) for c, segs, _ in fuzz if c["kind"] == "scattered"]
    assert min(scattered) < gc.PAIR_LIMIT < max(scattered)            # both sides of the table's size
    ragged = [len({int(s.max()) + 1 for s in segs}) for _, segs, _ in fuzz]
    assert max(ragged) >= 3
