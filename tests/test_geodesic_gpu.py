"""Geodesic click hints on the MI355X: ggc_geodesic_hints, the pipeline, the click evaluation, GrabCut.add_hints and the
CLI, every comparison array_equal against tests/geodesic_ref.py (a heapq Dijkstra written from the header's contract)."""
import subprocess
import sys
from dataclasses import replace
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

from geodesic_ref import definite_labels, geodesic_ref, serpentine
from helpers import seeded_state_dict
from test_hints_gpu import _block_segments, _random_clicks

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
H, W = 37, 53
SETTINGS = [(0, 0), (0, 12), (2, 12), (2, 40), (7, 64), (64, 16384)]      # (gamma, radius)


# ---------------------------------------------------------------- the kernel

@lru_cache(maxsize=None)
def _kernel_batch():
    """Six 37x53 images (no tile multiple) with random masks and block label maps.  Image 0 has a pixel clicked with both
    labels (and one clicked twice with the same), image 3 only background clicks, image 5 none."""
    from gcn_grabcut.synthetic import synthetic_image
    rng = np.random.default_rng(11)
    imgs = np.stack([synthetic_image(H, W, s) for s in range(1, 7)])
    masks = rng.integers(0, 4, (6, H, W)).astype(np.uint8)
    segs = np.stack([_block_segments(rng, H, W) for _ in range(6)])
    per_image = []
    for b in range(6):
        if b == 5:
            per_image.append(None)
            continue
        n = int(rng.integers(1, 41)) if b else 12
        pts = _random_clicks(rng, H, W, n)
        k = 0 if b == 3 else int(rng.integers(1, n + 1))
        fg, bg = pts[:k], pts[k:]
        if b == 0:
            fg, bg = fg + [(10, 10), (20, 31), (20, 31)], bg + [(10, 10), (30, 5)]
        per_image.append((fg, bg))
    return imgs, masks, segs, per_image


@lru_cache(maxsize=None)
def _want(b, gamma, radius):
    imgs, masks, segs, per_image = _kernel_batch()
    fg, bg = per_image[b] if per_image[b] is not None else ([], [])
    return geodesic_ref(imgs[b], fg, bg, radius, gamma, mask=masks[b], segments=segs[b])


def _call(eng, imgs, per_image, radius, gamma, masks=None, segs=None, want=("mask", "dist_fg", "dist_bg", "node_dist"),
          sentinel=-7):
    """Runs ggc_geodesic_hints on a batch; returns the requested outputs as NumPy arrays (node_dist split per image)."""
    from gcn_grabcut.graph_builder import pack_hints
    b, h, w = imgs.shape[:3]
    rows, ptr = pack_hints(per_image)
    hints, hint_ptr = eng.upload_hints(rows, ptr)
    bgr = eng.to_device(np.ascontiguousarray(imgs))
    kw, out = {}, {}
    if "mask" in want:
        kw["mask"] = eng.to_device(masks)
    for k in ("dist_fg", "dist_bg"):
        if k in want:
            kw[k] = torch.full((b, h, w), sentinel, dtype=torch.int32, device=eng.device)
    node_ptr = None
    if "node_dist" in want:
        node_ptr = np.concatenate([[0], np.cumsum([int(s.max()) + 1 for s in segs])]).astype(np.int32)
        kw["segments"] = eng.to_device(segs.astype(np.int32))
        kw["node_ptr"] = eng.to_device(node_ptr)
        kw["node_dist"] = torch.full((int(node_ptr[-1]), 2), sentinel, dtype=torch.int32, device=eng.device)
    eng.geodesic_hints(bgr, hints, hint_ptr, radius, gamma, **kw)
    for k in want:
        out[k] = kw[k].cpu().numpy()
    if node_ptr is not None:
        out["node_dist"] = [out["node_dist"][node_ptr[i]:node_ptr[i + 1]] for i in range(b)]
    return out


@pytest.fixture(scope="module")
def eng():
    from gcn_grabcut._engine import get_engine
    return get_engine("cuda")


@pytest.fixture(scope="module")
def batch_runs(eng):
    imgs, masks, segs, per_image = _kernel_batch()
    return {(g, r): _call(eng, imgs, per_image, r, g, masks, segs) for g, r in SETTINGS}


@pytest.mark.parametrize("gamma,radius", SETTINGS)
def test_kernel_batch_matches_the_reference(batch_runs, gamma, radius):
    imgs, masks, segs, per_image = _kernel_batch()
    got = batch_runs[(gamma, radius)]
    limit = 80 * radius
    for b in range(6):
        want = _want(b, gamma, radius)
        for k in ("dist_fg", "dist_bg", "mask"):
            assert np.array_equal(got[k][b], want[k]), (b, k)
        assert np.array_equal(got["node_dist"][b], want["node_dist"]), b
    assert np.array_equal(got["mask"][5], masks[5])
    assert (got["dist_fg"][3] == limit + 1).all() and (got["dist_fg"][5] == limit + 1).all()
    if radius == 12:                                                    # the cap cuts the frame: reached and unreached pixels
        d = got["dist_fg"][1]
        assert (d <= limit).any() and (d == limit + 1).any()


def test_doubly_clicked_pixel_takes_the_last_label(batch_runs):
    got = batch_runs[(2, 12)]
    assert got["dist_bg"][0][10, 10] == 0 and got["dist_fg"][0][10, 10] > 0 and got["mask"][0][10, 10] == 0
    assert got["dist_fg"][0][20, 31] == 0 and got["mask"][0][20, 31] == 1


@pytest.fixture(scope="module")
def serpentine_want():
    img = serpentine()
    return img, geodesic_ref(img, [(1, 1)], [], 4000, 16)


def test_serpentine_alone_and_in_a_batch(eng, serpentine_want):
    """A path that winds through the 3x3 tiles 11 times: a relaxation that stops early or reads a stale halo shows here."""
    from gcn_grabcut.synthetic import synthetic_image
    img, want = serpentine_want
    assert want["dist_fg"][68, 1] == 66839
    alone = _call(eng, img[None], [([(1, 1)], [])], 4000, 16, want=("dist_fg", "dist_bg"))
    assert np.array_equal(alone["dist_fg"][0], want["dist_fg"])
    assert np.array_equal(alone["dist_bg"][0], want["dist_bg"])
    imgs = np.stack([synthetic_image(70, 70, 1), synthetic_image(70, 70, 2), img])
    per_image = [([(5, 5)], [(60, 60)]), None, ([(1, 1)], [])]
    got = _call(eng, imgs, per_image, 4000, 16, want=("dist_fg", "dist_bg"))
    assert np.array_equal(got["dist_fg"][2], want["dist_fg"])
    assert np.array_equal(got["dist_bg"][2], want["dist_bg"])
    first = geodesic_ref(imgs[0], [(5, 5)], [(60, 60)], 4000, 16)
    assert np.array_equal(got["dist_fg"][0], first["dist_fg"]) and np.array_equal(got["dist_bg"][0], first["dist_bg"])


@pytest.mark.parametrize("h,w", [(1, 1), (1, 70), (70, 1), (33, 65), (64, 64)])
def test_shapes_with_a_click_on_the_last_pixel(eng, h, w):
    from gcn_grabcut.synthetic import synthetic_image
    img = synthetic_image(max(h, 8), max(w, 8), 21)[:h, :w]
    mask = np.full((1, h, w), 2, np.uint8)
    fg, bg = [(h - 1, w - 1)], [(0, 0)] if h * w > 1 else []
    got = _call(eng, img[None], [(fg, bg)], 70, 1, mask, want=("mask", "dist_fg", "dist_bg"))
    want = geodesic_ref(img, fg, bg, 70, 1, mask=mask[0])
    for k in ("mask", "dist_fg", "dist_bg"):
        assert np.array_equal(got[k][0], want[k]), k
    assert got["dist_fg"][0][h - 1, w - 1] == 0


@pytest.mark.parametrize("gamma,radius", [(64, 200), (2, 40), (0, 3)])
def test_sources_on_tile_corners_and_edges(eng, gamma, radius):
    """A source on the border of its 32x32 tile is seen by the neighbouring tiles although no visit ever lowers it."""
    from gcn_grabcut.synthetic import synthetic_image
    img = synthetic_image(70, 70, 5)
    cases = [([(31, 31)], [(32, 32)]), ([(31, 32), (0, 31)], [(63, 64)]), ([(32, 31)], [])]
    imgs = np.stack([img] * 3)
    masks = np.full((3, 70, 70), 2, np.uint8)
    got = _call(eng, imgs, cases, radius, gamma, masks, want=("mask", "dist_fg", "dist_bg"))
    for b, (fg, bg) in enumerate(cases):
        want = geodesic_ref(img, fg, bg, radius, gamma, mask=masks[b])
        for k in ("mask", "dist_fg", "dist_bg"):
            assert np.array_equal(got[k][b], want[k]), (b, k)


def test_every_image_equals_its_single_image_call_and_runs_repeat(eng, batch_runs):
    imgs, masks, segs, per_image = _kernel_batch()
    ref = batch_runs[(2, 40)]
    again = _call(eng, imgs, per_image, 40, 2, masks, segs)
    for k in ("mask", "dist_fg", "dist_bg"):
        assert np.array_equal(again[k], ref[k]), k
    for b in range(6):
        one = _call(eng, imgs[b:b + 1], [per_image[b]], 40, 2, masks[b:b + 1], segs[b:b + 1],
                    sentinel=80 * 40 + 1)                               # an image without clicks writes nothing: the cap
        for k in ("mask", "dist_fg", "dist_bg"):
            assert np.array_equal(one[k][0], ref[k][b]), (b, k)
        if per_image[b] is not None:
            assert np.array_equal(one["node_dist"][0], ref["node_dist"][b]), b


def test_null_outputs_and_argument_checks(eng, batch_runs):
    from gcn_grabcut import _native
    imgs, masks, segs, per_image = _kernel_batch()
    ref = batch_runs[(2, 12)]
    names = ("mask", "dist_fg", "dist_bg", "node_dist")
    for bits in range(1, 15):
        want = tuple(n for i, n in enumerate(names) if (bits >> i) & 1)
        got = _call(eng, imgs, per_image, 12, 2, masks, segs, want=want)
        for k in want:
            if k == "node_dist":
                assert all(np.array_equal(a, b) for a, b in zip(got[k], ref[k])), want
            else:
                assert np.array_equal(got[k], ref[k]), (want, k)
    bgr = eng.to_device(imgs)
    m = eng.to_device(masks)
    hints, ptr = eng.upload_hints(np.array([[1, 1, 1]], np.int32), np.array([0, 1, 1, 1, 1, 1, 1], np.int32))
    with pytest.raises(_native.GGCError, match="INVALID_ARG"):
        eng.geodesic_hints(bgr, hints, ptr, 12, 2)                      # no output at all
    for radius, gamma in ((-1, 2), (16385, 2), (12, -1), (12, 65)):
        with pytest.raises(_native.GGCError, match="INVALID_ARG"):
            eng.geodesic_hints(bgr, hints, ptr, radius, gamma, mask=m)
    for bad in ([0, 2, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1]):
        _, bad_ptr = eng.upload_hints(np.array([[1, 1, 1]] * 2, np.int32), np.array(bad, np.int32))
        with pytest.raises(_native.GGCError, match="INVALID_ARG"):
            eng.geodesic_hints(bgr, hints, bad_ptr, 12, 2, mask=m)
    assert torch.equal(m, eng.to_device(masks))                         # nothing was launched
    _, empty = eng.upload_hints(np.zeros((0, 3), np.int32), np.zeros(7, np.int32))
    df = torch.full((6, H, W), -7, dtype=torch.int32, device=eng.device)
    db = df.clone()
    eng.geodesic_hints(bgr, None, empty, 12, 2, mask=m, dist_fg=df, dist_bg=db)   # K == 0 writes nothing
    assert torch.equal(m, eng.to_device(masks)) and bool((df == -7).all()) and bool((db == -7).all())


# ---------------------------------------------------------------- pipeline, click evaluation, GrabCut, CLI

PH, PW = 96, 128
KEYS = ("binary_mask", "trimap", "segments", "probs", "gc_mask", "overlay", "rgba")


def _scene_hints():
    return [([(40, 60), (PH - 1, PW - 1)], [(3, 3), (41, 66), (-5, 2)]), None,
            ([(PH // 2, PW // 2)], [(PH // 2, PW // 2 + 9), (0, PW - 2)]), ([], [(10, 100)])]


@pytest.fixture(scope="module")
def scenes():
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig
    from gcn_grabcut.synthetic import synthetic_image
    model, _ = seeded_state_dict(32, 2, seed=5)
    pipe = GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=60), device="cuda")
    pairs = [synthetic_image(PH, PW, 700 + i, return_mask=True) for i in range(4)]
    imgs, gts = [p[0] for p in pairs], [p[1] for p in pairs]
    bgr = pipe._eng.to_device(np.stack(imgs))
    hints = _scene_hints()
    base = pipe.segment_batch_device(bgr, chunks=1)
    geo = pipe.segment_batch_device(bgr, chunks=1, hints=hints, geodesic=True, hint_radius=1)
    return pipe, imgs, gts, bgr, hints, base, geo


def test_pipeline_paints_the_trimap_as_the_reference_does(scenes):
    pipe, imgs, gts, bgr, hints, base, geo = scenes
    for b in range(4):
        tri0 = base["trimap"][b].cpu().numpy()
        if hints[b] is None:
            for k in ("binary_mask", "trimap", "gc_mask"):
                assert torch.equal(base[k][b], geo[k][b]), (b, k)
            continue
        want = geodesic_ref(imgs[b], *hints[b], 40, 2, mask=tri0)["mask"]
        assert np.array_equal(geo["trimap"][b].cpu().numpy(), want), b
        lab = definite_labels(imgs[b], *hints[b], 40, 2)
        assert (lab >= 0).sum() > 81                                    # more than the r = 5 disk of one click
        m = geo["gc_mask"][b].cpu().numpy()
        assert (m[lab == 1] == 1).all() and (m[lab == 0] == 0).all(), b
    assert torch.equal(base["probs"], geo["probs"])                     # hard constraints do not touch the network
    with pytest.raises(ValueError, match="hint_region"):
        pipe.segment_batch_device(bgr, hints=hints, geodesic=True, hint_region=True)
    off = pipe.segment_batch_device(bgr, chunks=1, geodesic=True)       # no clicks: what a call without the option gives
    for k in KEYS:
        assert torch.equal(off[k], base[k]), k


def test_pipeline_chunked_equals_one_chunk_and_segment(scenes):
    from gcn_grabcut import GeodesicHints
    pipe, imgs, gts, bgr, hints, base, geo = scenes
    two = pipe.segment_batch_device(bgr, chunks=2, hints=hints, geodesic=GeodesicHints())
    for k in KEYS:
        assert torch.equal(geo[k], two[k]), k
    r = pipe.segment(imgs[2], fg_points=hints[2][0], bg_points=hints[2][1], geodesic=True)
    assert np.array_equal(r.trimap, geo["trimap"][2].cpu().numpy())
    one = pipe.segment_batch_device(bgr[2:3], hints=[hints[2]], geodesic=True)   # GrabCut runs image b on seed + b
    assert np.array_equal(r.trimap, one["trimap"][0].cpu().numpy())
    assert np.array_equal(r.binary_mask, one["binary_mask"][0].cpu().numpy())

def test_pipeline_soft_prior_columns(scenes):
    from gcn_grabcut import GeodesicHints, encode_geodesic_hints
    pipe, imgs, gts, bgr, hints, base, geo = scenes
    g = GeodesicHints(30, 3, 6.0)
    out = pipe.segment_batch_device(bgr, chunks=1, hints=hints, geodesic=g, hints_as_prior=True)
    gr = base["graphs"]
    x = gr.x.clone()
    seg = base["segments"].cpu().numpy()
    for b in range(4):
        n0, n1 = gr.node_ptr_host[b], gr.node_ptr_host[b + 1]
        if hints[b] is None:
            continue
        cols = encode_geodesic_hints(imgs[b], seg[b], *hints[b], geodesic=g)
        nd = geodesic_ref(imgs[b], *hints[b], g.radius, g.gamma, segments=seg[b])["node_dist"].astype(np.float64)
        e = np.where(nd > 80 * g.radius, 0.0, np.exp(-nd / (80.0 * g.sigma)))
        want = np.concatenate([e, 1.0 - e.max(1, keepdims=True)], 1).astype(np.float32)
        assert np.array_equal(cols, want), b
        assert 0.0 < cols[:, 0].max() <= 1.0 or 0.0 < cols[:, 1].max() <= 1.0
        x[n0:n1, 16:19] = torch.from_numpy(cols).to(x.device)
    assert torch.equal(out["graphs"].x, x)
    assert torch.equal(out["probs"], pipe._eng.predict_probs(pipe.model, replace(gr, x=x)))
    assert np.array_equal(encode_geodesic_hints(imgs[1], seg[1], [], []),
                          np.tile(np.array([0, 0, 1], np.float32), (int(seg[1].max()) + 1, 1)))


@pytest.fixture(scope="module")
def click_runs(scenes):
    pipe, imgs, gts, bgr, hints, base, geo = scenes
    return pipe.evaluate_clicks(imgs, gts, max_clicks=3, geodesic=True, return_masks=True)


def test_evaluate_clicks_masks_carry_the_reference_labels_of_all_clicks_so_far(scenes, click_runs):
    pipe, imgs, gts, bgr, hints, base, geo = scenes
    full = click_runs
    assert full["masks"].shape == (4, 4, PH, PW)
    painted = 0
    for i in range(4):
        for k in range(1, len(full["clicks"][i]) + 1):
            lab = definite_labels(imgs[i], None, None, 40, 2, rows=full["clicks"][i][:k])
            m = full["masks"][i, k]
            assert (m[lab == 1] == 1).all() and (m[lab == 0] == 0).all(), (i, k)
            painted += int((lab >= 0).sum())
    assert painted > 0


def test_evaluate_clicks_batch_equals_one_image_calls(scenes, click_runs):
    pipe, imgs, gts, bgr, hints, base, geo = scenes
    from gcn_grabcut import GCNGrabCutPipeline
    stop = float(np.sort(click_runs["ious"][:3, 1])[1])                 # at least one of the three stops after a click
    # the automatic pass runs image b of a batch on GrabCutConfig.seed + b (segment_batch_device), so the one-image call
    # that image i's row of the batch must equal is the one on seed + i
    alone = [GCNGrabCutPipeline(pipe.model, pipe.sp_config, replace(pipe.gc_config, seed=pipe.gc_config.seed + i),
                                device="cuda") for i in range(3)]
    for kw in ({}, {"stop_iou": stop}):
        three = pipe.evaluate_clicks(imgs[:3], gts[:3], max_clicks=3, geodesic=True, **kw)
        if not kw:
            assert three["clicks"] == click_runs["clicks"][:3] and np.array_equal(three["ious"], click_runs["ious"][:3])
        for i in range(3):
            one = alone[i].evaluate_clicks(imgs[i:i + 1], gts[i:i + 1], max_clicks=3, geodesic=True, **kw)
            assert one["clicks"][0] == three["clicks"][i], (i, kw)
            assert np.array_equal(one["ious"][0], three["ious"][i]), (i, kw)


def test_grabcut_add_hints_geodesic_then_refine():
    from gcn_grabcut import GeodesicHints, GrabCut
    from gcn_grabcut.synthetic import synthetic_image
    img = synthetic_image(70, 90, 1234)
    gc = GrabCut(img, device="cuda")
    tri = np.full((70, 90), 2, np.uint8)
    tri[20:50, 25:65] = 3
    tri[30:40, 35:55] = 1
    tri[:4] = 0
    gc.run_with_trimap(tri)
    m0 = gc.mask.copy()
    fg, bg = [(60, 10), (8, 80)], [(35, 45), (62, 14)]
    gc.add_hints(fg_points=fg, bg_points=bg, geodesic=GeodesicHints(20, 2))
    assert np.array_equal(gc.mask, geodesic_ref(img, fg, bg, 20, 2, mask=m0)["mask"])
    assert gc.history[-1].tag == "hints"
    gc.refine(1)
    lab = definite_labels(img, fg, bg, 20, 2)
    assert (lab == 1).sum() > 2 and (lab == 0).sum() > 2
    assert (gc.mask[lab == 1] == 1).all() and (gc.mask[lab == 0] == 0).all()


def test_geodesic_hints_function(eng):
    from gcn_grabcut import geodesic_hints
    from gcn_grabcut.synthetic import synthetic_image
    img = synthetic_image(50, 60, 77)
    want = geodesic_ref(img, [(20, 20)], [(45, 5)], 15, 3, mask=np.full((50, 60), 2, np.uint8))
    assert np.array_equal(geodesic_hints(img, [(20, 20)], [(45, 5)], 15, 3), want["mask"])
    df, db = geodesic_hints(img, [(20, 20)], [(45, 5)], 15, 3, return_dist=True)
    assert np.array_equal(df, want["dist_fg"]) and np.array_equal(db, want["dist_bg"])


def test_cli_geodesic_mode_runs_and_keeps_the_clicks(tmp_path):
    from PIL import Image
    from gcn_grabcut.synthetic import synthetic_image
    img = synthetic_image(150, 200, 4242)
    Image.fromarray(img[:, :, ::-1]).save(tmp_path / "x.png")
    model, sd = seeded_state_dict(32, 2, seed=8)
    torch.save({"model": sd, "epoch": 1}, tmp_path / "ckpt.pt")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--image", str(tmp_path / "x.png"), "--output", str(out),
                        "--checkpoint", str(tmp_path / "ckpt.pt"), "--superpixels", "100", "--min-area", "0", "--save", "mask",
                        "--fg-point", "50,75", "--bg-point", "125,20", "--hint-mode", "geodesic", "--hint-gamma", "2",
                        "--geodesic-radius", "25"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    mask = np.asarray(Image.open(out / "x_mask.png"))
    assert mask.shape == (150, 200)
    lab = definite_labels(img, [(50, 75)], [(125, 20)], 25, 2)
    assert (mask[lab == 1] == 255).all() and (mask[lab == 0] == 0).all()
