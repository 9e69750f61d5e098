"""Geodesic click hints without a GPU: the NumPy reference (tests/geodesic_ref.py) against SciPy's Dijkstra, a closed form
and a winding scene; what the definition is worth on the synthetic scenes; sources, validation, header and CLI flags."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from geodesic_ref import (AXIAL, DIAG, definite_labels, distances, geodesic_ref, guide, serpentine, sources)

ROOT = Path(__file__).resolve().parent.parent


def _explicit_graph(img, gamma):
    """The definition's graph as a SciPy sparse matrix: one entry per arc of the 8-connected grid."""
    from scipy.sparse import coo_matrix
    h, w = img.shape[:2]
    s = np.zeros((h, w, 3), np.int64)
    for y in range(h):                                                  # the box sum, spelled out
        for x in range(w):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    s[y, x] += img[min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)]
    assert np.array_equal(s, guide(img))
    idx = np.arange(h * w).reshape(h, w)
    rows, cols, vals = [], [], []
    for dy, dx, length in ((0, 1, AXIAL), (1, 0, AXIAL), (1, 1, DIAG), (1, -1, DIAG)):
        ys, xs = np.mgrid[0:h - dy, max(0, -dx):w - max(0, dx)]
        c = length + gamma * np.abs(s[ys, xs] - s[ys + dy, xs + dx]).sum(-1)
        rows += [idx[ys, xs].ravel(), idx[ys + dy, xs + dx].ravel()]
        cols += [idx[ys + dy, xs + dx].ravel(), idx[ys, xs].ravel()]
        vals += [c.ravel(), c.ravel()]
    return coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(h * w, h * w)).tocsr()


@pytest.mark.parametrize("gamma", [0, 2])
def test_reference_agrees_with_scipy_dijkstra(gamma):
    from scipy.sparse.csgraph import dijkstra
    from gcn_grabcut.synthetic import synthetic_image
    img = synthetic_image(37, 53, 7)
    srcs = [(0, 0), (36, 52), (18, 30)]
    limit = AXIAL * 12
    d = dijkstra(_explicit_graph(img, gamma), directed=True, indices=[r * 53 + c for r, c in srcs], min_only=True)
    want = np.minimum(d, limit + 1).astype(np.int32).reshape(37, 53)
    got = distances(img, srcs, 12, gamma)
    assert np.array_equal(got, want)
    assert (got <= limit).any() and (got == limit + 1).any()            # the cap binds on a part of the frame


def test_flat_image_gives_the_closed_form():
    img = np.full((70, 70, 3), 90, np.uint8)
    rng = np.random.default_rng(0)
    img2 = rng.integers(0, 256, (70, 70, 3)).astype(np.uint8)          # gamma = 0: the image does not matter
    yy, xx = np.mgrid[0:70, 0:70]
    a, b = np.abs(yy - 10), np.abs(xx - 20)
    want = AXIAL * (np.maximum(a, b) - np.minimum(a, b)) + DIAG * np.minimum(a, b)
    for im in (img, img2):
        assert np.array_equal(distances(im, [(10, 20)], 2000, 0), want)


@pytest.mark.parametrize("gamma", [2, 16, 64])
def test_serpentine_path_goes_round_every_wall(gamma):
    d = distances(serpentine(), [(1, 1)], 4000, gamma)
    assert d[68, 1] == 66839                                            # 835.4875 x 80, against 68 x 80 for the straight line
    assert d[1, 1] == 0 and d[68, 68] <= 80 * 4000


def _edt_max(region):
    from scipy import ndimage
    e = ndimage.distance_transform_edt(np.pad(region, 1))[1:-1, 1:-1]
    return tuple(int(v) for v in np.unravel_index(e.argmax(), e.shape))


@pytest.mark.parametrize("seed", [30000, 30001, 30002, 30003])
def test_one_click_labels_hundreds_of_pixels_and_none_outside_the_object(seed):
    from gcn_grabcut.synthetic import synthetic_image
    img, gt = synthetic_image(120, 160, seed, return_mask=True)
    lab = definite_labels(img, [_edt_max(gt)], [_edt_max(1 - gt)], 30, 2)
    n_fg, wrong = int((lab == 1).sum()), int(((lab == 1) & (gt == 0)).sum())
    print(f"seed {seed}: {n_fg} pixels foreground, {wrong} outside the ground truth")
    assert n_fg > 400
    assert wrong == 0


def test_sources_last_click_wins_and_out_of_frame_clicks_are_ignored():
    fg, bg = sources(20, 30, [(5, 5), (7, 7), (-1, 3), (20, 0)], [(5, 5), (3, 30), (8, 8)])
    assert sorted(fg) == [(7, 7)] and sorted(bg) == [(5, 5), (8, 8)]    # pack_hints puts background clicks last
    img = np.full((20, 30, 3), 100, np.uint8)
    mask = np.full((20, 30), 3, np.uint8)
    out = geodesic_ref(img, [(5, 5)], [(5, 5)], 3, 2, mask=mask)
    assert out["mask"][5, 5] == 0 and out["dist_bg"][5, 5] == 0 and (out["dist_fg"] == 241).all()
    rows = [(5, 5, 0), (5, 5, 1)]                                       # the other order: the foreground click is the last
    assert geodesic_ref(img, None, None, 3, 2, mask=mask, rows=rows)["mask"][5, 5] == 1
    none = geodesic_ref(img, [(-2, 0)], [(0, 30)], 3, 2, mask=mask, segments=np.zeros((20, 30), np.int32))
    assert np.array_equal(none["mask"], mask) and (none["dist_fg"] == 241).all() and (none["dist_bg"] == 241).all()
    assert none["node_dist"].tolist() == [[241, 241]]


def test_ties_and_the_limit():
    img = np.full((1, 9, 3), 50, np.uint8)
    mask = np.full((1, 9), 2, np.uint8)
    out = geodesic_ref(img, [(0, 0)], [(0, 8)], 3, 5, mask=mask)        # both reach 3 pixels; the middle is out of reach
    assert out["mask"].tolist() == [[1, 1, 1, 1, 2, 0, 0, 0, 0]]
    assert out["dist_fg"].tolist() == [[0, 80, 160, 240, 241, 241, 241, 241, 241]]
    out = geodesic_ref(img, [(0, 0)], [(0, 8)], 5, 5, mask=mask)        # the pixel at equal distance is left alone
    assert out["mask"].tolist() == [[1, 1, 1, 1, 2, 0, 0, 0, 0]] and out["dist_fg"][0, 4] == out["dist_bg"][0, 4] == 320


def test_geodesic_hints_validates_its_ranges():
    from gcn_grabcut import GeodesicHints
    g = GeodesicHints()
    assert (g.radius, g.gamma, g.sigma) == (40, 2, 10.0)
    GeodesicHints(0, 0), GeodesicHints(16384, 64)
    for kw in (dict(radius=-1), dict(radius=16385), dict(gamma=-1), dict(gamma=65), dict(radius=2.5), dict(sigma=0.0),
               dict(sigma=float("nan"))):
        with pytest.raises(ValueError):
            GeodesicHints(**kw)


def test_geodesic_with_hint_region_is_refused_and_no_clicks_is_a_no_op():
    from gcn_grabcut import GeodesicHints
    from gcn_grabcut.pipeline import _Hints, _geodesic_args
    clicks = [([(1, 1)], [])]
    with pytest.raises(ValueError, match="hint_region"):
        _Hints.of(clicks, 1, 5, True, False, geodesic=True)
    with pytest.raises(ValueError, match="hint_region"):
        _Hints.of(None, 1, 5, True, False, geodesic=GeodesicHints())
    with pytest.raises(ValueError):
        _geodesic_args("yes")
    assert _Hints.of(None, 1, 5, False, False, geodesic=True) is None   # nothing to launch
    assert _Hints.of([None], 1, 5, False, False, geodesic=True) is None
    h = _Hints.of(clicks + [None], 2, 5, False, True, geodesic=GeodesicHints(7, 3))
    assert h.geodesic == GeodesicHints(7, 3) and h.chunk(0, 1).geodesic == h.geodesic and h.chunk(1, 2) is None
    assert _Hints.of(clicks, 1, 5, False, False).geodesic is None       # off by default


def test_soft_prior_columns():
    from gcn_grabcut.graph_builder import geodesic_prior_columns
    nd = np.array([[0, 3201], [800, 1600], [3201, 3201], [3200, 0]], np.int32)
    got = geodesic_prior_columns(nd, 40, 10.0)
    e = lambda d: np.exp(-d / 800.0)
    want = np.array([[1.0, 0.0, 0.0], [e(800), e(1600), 1 - e(800)], [0.0, 0.0, 1.0], [e(3200), 1.0, 0.0]]).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_header_exports_and_cli_flags():
    from gcn_grabcut import _native
    import gcn_grabcut
    header = (ROOT / "include" / "ggc.h").read_text()
    assert int(re.search(r"#define GGC_VERSION (\d+)", header).group(1)) >= 404
    assert "ggc_geodesic_hints" in header
    assert len(_native.SIGNATURES["ggc_geodesic_hints"]) == 16
    for name in ("GeodesicHints", "geodesic_hints", "encode_geodesic_hints"):
        assert name in gcn_grabcut.__all__ and hasattr(gcn_grabcut, name)
    sys.path.insert(0, str(ROOT))
    import evaluate_clicks
    import inference
    a = inference.build_parser().parse_args(["--image", "x.png"])
    assert (a.hint_mode, a.hint_gamma, a.geodesic_radius) == ("disk", 2, 40)
    a = inference.build_parser().parse_args(["--image", "x.png", "--hint-mode", "geodesic", "--hint-gamma", "5",
                                             "--geodesic-radius", "60"])
    assert (a.hint_mode, a.hint_gamma, a.geodesic_radius) == ("geodesic", 5, 60)
    a = evaluate_clicks.build_parser().parse_args(["--images", "i", "--masks", "m", "--hint-mode", "geodesic",
                                                   "--hint-gamma", "3", "--geodesic-radius", "25"])
    assert (a.hint_mode, a.hint_gamma, a.geodesic_radius) == ("geodesic", 3, 25)
    assert evaluate_clicks.build_parser().parse_args(["--images", "i", "--masks", "m"]).hint_mode == "disk"
