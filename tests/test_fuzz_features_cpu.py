"""The feature fuzzer (tests/fuzz_features.py) checked without a GPU, for every family and the seeds the device pass uses:
its case lists are deterministic, inside the limits of include/ggc.h, walk every tile and wave boundary, and are not
vacuous; the ties and caps that the entries' rules single out do occur.  Everything here comes from the generators and the
references alone."""
import numpy as np
import pytest

import fuzz_features as ff
from test_hints_gpu import disk_labels
from test_next_click_gpu import region_d2

SEEDS = ff.SUITE_SEEDS
PRIMITIVES = ("clicks", "geodesic", "strokes", "stroke_pixels", "polygons", "scissors")
LIMIT = 1 << 20


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return type(a) is type(b) and a == b


def _refs(family, seed, orc):
    return [ff.suite_reference(family, seed, i, orc) for i in range(ff.N_CASES)]


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_case_lists_are_deterministic(family):
    for seed in SEEDS:
        first, again = ff.make_cases(family, seed), ff.make_cases(family, seed)
        assert len(first) == ff.N_CASES and _same(first, again), (family, seed)
        assert _same(first[17], ff.make_case(family, seed, 17))         # case i depends on (family, seed, i) only
    assert not _same(ff.make_case(family, SEEDS[0], 30), ff.make_case(family, SEEDS[1], 30))
    assert _same(ff.make_case("stroke_pixels", 5, 9)["per_image"], ff.make_case("strokes", 5, 9)["per_image"])


# ---------------------------------------------------------------- validity: the limits of include/ggc.h

def _check_ptr(ptr, total, groups):
    ptr = np.asarray(ptr)
    assert ptr.dtype == np.int32 and len(ptr) == groups + 1 and ptr[0] == 0 and (np.diff(ptr) >= 0).all() and ptr[-1] == total


def _check_clicks(c):
    assert len(c["per_image"]) == c["b"]
    for i, entry in enumerate(c["per_image"]):
        assert (entry is None) == (i == c["empty"])
        for r, col in (entry or ([], []))[0] + (entry or ([], []))[1]:
            assert -4 <= r <= c["h"] + 12 and -4 <= col <= c["w"] + 12
    for seg in c["segs"]:
        assert seg.min() == 0 and len(np.unique(seg)) == seg.max() + 1  # labels 0..n-1, all present


def _valid_clicks(c):
    assert c["params"]["radius"] in (0, 1, 3, 7, 40) and c["params"]["region"] in (0, 1)
    assert 1 <= sum(len(e[0]) + len(e[1]) for e in c["per_image"] if e) <= 40 * c["b"]
    assert c["masks"].dtype == np.uint8 and c["masks"].max() <= 3
    _check_clicks(c)


def _valid_geodesic(c):
    p = c["params"]
    assert 0 <= p["radius"] <= 16384 and 0 <= p["gamma"] <= 64 and (p["gamma"], p["radius"]) in ff.geodesic_tests.SETTINGS
    assert 1 <= len(c["outputs"]) <= 4 and set(c["outputs"]) <= {"mask", "dist_fg", "dist_bg", "node_dist"}
    assert c["imgs"].shape == (c["b"], c["h"], c["w"], 3) and c["imgs"].dtype == np.uint8
    assert all(len(e[0]) + len(e[1]) <= 12 for e in c["per_image"] if e)
    _check_clicks(c)


def _valid_strokes(c):
    assert c["params"]["radius"] in (0, 1, 3, 9, 40)
    for i, segs in enumerate(c["per_image"]):
        assert (len(segs) == 0) == (i == c["empty"]) and len(segs) <= 30
        for r0, c0, r1, c1, label in segs:
            assert max(abs(r0), abs(c0), abs(r1), abs(c1)) <= LIMIT and label in (0, 1)
    strokes, ptr = ff.strokes_ref.pack(c["per_image"])
    _check_ptr(ptr, len(strokes), c["b"])


def _valid_polygons(c):
    verts, poly_ptr, labels, image_ptr = c["packed"]
    _check_ptr(poly_ptr, len(verts), len(labels))
    _check_ptr(image_ptr, len(labels), c["b"])
    assert len(labels) >= 1 and set(labels.tolist()) <= {0, 1, 2} and np.abs(verts).max() <= LIMIT
    assert ((np.diff(poly_ptr) >= 3) & (np.diff(poly_ptr) <= 8)).all() and (np.diff(image_ptr) <= 5).all()
    assert [int(n) == 0 for n in np.diff(image_ptr)] == [i == c["empty"] for i in range(c["b"])]


def _valid_scissors(c):
    from gcn_grabcut.graph_builder import pack_paths
    margin, edge_cap, smooth = c["setting"]
    assert 0 <= margin <= 256 and 1 <= edge_cap <= 13770 and 1 <= smooth <= 64
    for i, paths in enumerate(c["paths"]):
        assert (paths is None) == (i == c["empty"])
        for pts, closed in paths or []:
            assert (3 if closed else 2) <= len(pts) <= 6
            assert all(0 <= r < c["h"] and 0 <= col < c["w"] for r, col in pts)                    # anchors inside the image
            assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) <= 1024 for a, b in ff.scissors_ref.segments(pts, closed))
    anchors, path_ptr, closed, image_ptr = pack_paths(c["paths"])
    _check_ptr(path_ptr, len(anchors), len(closed))
    _check_ptr(image_ptr, len(closed), c["b"])
    assert sum(ff.scissors_plane_sizes(c)) <= 1 << 26


def _valid_next_click(c):
    assert c["w"] <= 8192 and c["preds"].shape == c["gts"].shape == (c["b"], c["h"], c["w"])
    assert set(np.unique(c["gts"]).tolist()) <= {0, c["params"]["gt_scale"]} and c["preds"].max() <= 1
    assert c["empty"] is None or np.array_equal(c["preds"][c["empty"]] != 0, c["gts"][c["empty"]] != 0)   # no error: no click


def _valid_clean(c):
    assert c["masks"].dtype == np.uint8 and c["masks"].max() <= 1 and c["params"]["density"] in (0.05, 0.3, 0.6)
    assert c["empty"] is None or not c["masks"][c["empty"]].any()


def _valid_eval_counts(c):
    assert c["pred"].max() <= 1 and c["gt"].max() <= 1 and c["params"]["width"] in (0, 1, 3)
    assert (c["tri"] is None) == (not c["params"]["trimap"]) and (c["tri"] is None or c["tri"].max() <= 3)


def _valid_matte(c):
    assert c["a"].dtype == c["g"].dtype == np.uint8 and c["a"].shape == c["g"].shape == (c["b"], c["h"], c["w"])
    assert c["region"] is None or (c["region"].dtype == np.uint8 and c["region"].shape == c["a"].shape)


def _valid_seed_prior(c):
    assert c["params"]["seed_frac"] in (0.1, 0.25) and c["trimap"].dtype == np.uint8 and c["trimap"].max() <= 3
    _check_ptr(c["node_ptr"], len(c["prior"]), c["b"])
    assert c["prior"].dtype == np.float32 and c["prior"].shape[1] == 3 and 0.0 <= c["prior"].min() and c["prior"].max() <= 1.0
    for i, seg in enumerate(c["segs"]):
        assert seg.min() == 0 and len(np.unique(seg)) == seg.max() + 1 == c["node_ptr"][i + 1] - c["node_ptr"][i]


VALID = dict(mask_iou=_valid_eval_counts, seed_prior=_valid_seed_prior, clicks=_valid_clicks, geodesic=_valid_geodesic, strokes=_valid_strokes, stroke_pixels=_valid_strokes,
             polygons=_valid_polygons, scissors=_valid_scissors, next_click=_valid_next_click, clean=_valid_clean,
             eval_counts=_valid_eval_counts, matte=_valid_matte)


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_every_case_is_inside_the_headers_limits(family):
    for seed in SEEDS:
        for c in ff.suite_cases(family, seed):
            assert c["b"] in ff.BATCHES and 1 <= c["h"] <= 257 and 1 <= c["w"] <= 257
            assert (c["empty"] is None) == (c["b"] < 3)
            VALID[family](c)


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_the_schedule_walks_every_boundary(family):
    edges = ff.edges_of(family)
    assert set(ff.EDGES) <= set(edges) and (family not in ff.CHEAP or {255, 256, 257} <= set(edges))
    for seed in SEEDS:
        cases = ff.suite_cases(family, seed)
        assert [c["h"] for c in cases[1:len(edges)]] == edges[1:]       # the walk itself, not chance
        assert [c["w"] for c in cases[len(edges):2 * len(edges)]] == edges
        assert set(edges) <= {c["h"] for c in cases} and set(edges) <= {c["w"] for c in cases}
        assert any(c["b"] >= 3 for c in cases) and any(c["b"] == 1 for c in cases)
        assert any((c["h"], c["w"]) == (1, 1) for c in cases)
        assert family not in PRIMITIVES + ("clean", "next_click") or any(c["empty"] is not None for c in cases)
        assert any(c["h"] > 64 and c["w"] > 64 for c in cases)          # more than one tile both ways


# ---------------------------------------------------------------- non-vacuity, from the references alone

def _nontrivial(family, c, want):
    if family in ("clicks", "polygons"):
        return not np.array_equal(want["mask"], c["masks"])
    if family == "strokes":
        return not np.array_equal(want["mask"], c["masks"])
    if family == "stroke_pixels":
        return len(want["rows"]) > 0
    if family == "geodesic":
        limit = 80 * c["params"]["radius"]
        return any((f["dist_fg"] <= limit).any() or (f["dist_bg"] <= limit).any() for f in want["_full"])
    if family == "scissors":
        n_anchors = [len(pts) for paths in c["paths"] for pts, _ in paths or []]
        return bool((np.diff(want["count_ptr"]) > np.asarray(n_anchors)).any())
    if family == "next_click":
        return bool((want["click"][:, 0] >= 0).any())
    if family == "clean":
        return any(not np.array_equal(v, c["masks"]) for v in want.values())
    if family == "mask_iou":
        return bool((want["counts"] > 0).all(1).any())
    if family == "seed_prior":
        return not np.array_equal(want["trimap"], c["trimap"])          # some image had one side missing and got seeds
    if family == "eval_counts":
        return bool((want["counts"][:, :3] > 0).all(1).any())           # an image with true and false positives and misses
    return any(len(np.unique(lev)) > 1 for lev in want["levels"])       # matte: the level map is not constant


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_two_thirds_of_the_cases_are_not_trivial(family, oracle):
    for seed in SEEDS:
        cases, refs = ff.suite_cases(family, seed), _refs(family, seed, oracle)
        busy = sum(_nontrivial(family, c, r) for c, r in zip(cases, refs))
        assert 3 * busy >= 2 * len(cases), (family, seed, busy)


# ---------------------------------------------------------------- ties and caps

def test_geodesic_cases_hold_ties_and_capped_frames(oracle):
    for seed in SEEDS:
        ties = cut = 0
        for c, want in zip(ff.suite_cases("geodesic", seed), _refs("geodesic", seed, oracle)):
            limit = 80 * c["params"]["radius"]
            for f in want["_full"]:
                ties += bool(((f["dist_fg"] == f["dist_bg"]) & (f["dist_fg"] <= limit)).any())     # left untouched
                cut += any((d <= limit).any() and (d == limit + 1).any() for d in (f["dist_fg"], f["dist_bg"]))
        assert ties >= 1 and cut >= 1, (seed, ties, cut)


def test_click_cases_hold_pixels_under_disks_of_both_labels():
    for seed in SEEDS:
        both = 0
        for c in ff.suite_cases("clicks", seed):
            for entry in c["per_image"]:
                if entry:
                    fg = disk_labels(c["h"], c["w"], entry[0], [], c["params"]["radius"])
                    bg = disk_labels(c["h"], c["w"], [], entry[1], c["params"]["radius"])
                    both += bool(((fg >= 0) & (bg >= 0)).any())
        assert both >= 1, seed


def _on_an_edge(h, w, polygon):
    """(H,W) bool: rule (a) of H3, the pixels that lie on an edge of the polygon."""
    r, c = np.mgrid[0:h, 0:w].astype(np.int64)
    on = np.zeros((h, w), bool)
    for (ar, ac), (br, bc) in zip(polygon, polygon[1:] + polygon[:1]):
        on |= ((br - ar) * (c - ac) - (bc - ac) * (r - ar) == 0) & (min(ar, br) <= r) & (r <= max(ar, br)) \
            & (min(ac, bc) <= c) & (c <= max(ac, bc))
    return on


def test_polygon_cases_hold_pixels_exactly_on_an_edge():
    for seed in SEEDS:
        hit = 0
        for c in ff.suite_cases("polygons", seed):
            verts, poly_ptr, _, _ = c["packed"]
            for q in range(len(poly_ptr) - 1):
                poly = [tuple(int(x) for x in v) for v in verts[poly_ptr[q]:poly_ptr[q + 1]]]
                hit += bool(_on_an_edge(c["h"], c["w"], poly).any())
        assert hit >= 1, seed


def test_next_click_cases_hold_a_tie_of_the_two_maxima():
    for seed in SEEDS:
        ties = 0
        for c in ff.suite_cases("next_click", seed):
            for p, g in zip(c["preds"] != 0, c["gts"] != 0):
                m_fn, m_fp = int(region_d2(g & ~p).max()), int(region_d2(~g & p).max())
                ties += m_fn == m_fp > 0
        assert ties >= 1, seed


def test_the_chained_cases_occur(oracle):
    for seed in SEEDS:
        assert sum("lassoed" in r for r in _refs("scissors", seed, oracle)) >= ff.N_CASES // 4, seed
        assert sum(len(r["rows"]) > 0 for r in _refs("stroke_pixels", seed, oracle)) >= ff.N_CASES // 2, seed


def test_a_mismatch_is_one_replayable_line(oracle):
    case = ff.make_case("polygons", 3, 20)
    want = ff.reference(case, oracle)
    assert ff.compare(case, want, {k: v.copy() for k, v in want.items()}) == []
    wrong = want["mask"].copy()
    wrong[-1, -1, -1] ^= 1
    wrong[0, 0, 0] ^= 1
    (line,) = ff.compare(case, want, dict(mask=wrong))
    assert line.startswith(f"polygons seed=3 case=20 {case['b']}x{case['h']}x{case['w']} polygons=")
    assert "mask differs in 2 of" in line and "first at (0, 0, 0)" in line
    matte = ff.make_case("matte", 3, 20)
    want = ff.reference(matte, oracle)
    near = dict(want, grad=want["grad"] * (1.0 + 1e-12))
    far = dict(want, grad=want["grad"] + 1e-6 * (1.0 + want["grad"]))
    assert ff.compare(matte, want, near) == [] and len(ff.compare(matte, want, far)) == 1
