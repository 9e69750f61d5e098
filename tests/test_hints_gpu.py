"""Click guidance on the MI355X: ggc_apply_hints against a NumPy restatement of its semantics, the pipeline with hints
(hard constraints, chunked runs, hints as the network's prior), GrabCut.add_hints + refine, and the CLI's click flags."""
import subprocess
import sys
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import seeded_state_dict

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------- restatement of ggc_apply_hints (include/ggc.h, H0)

def paint(mask, seg, fg, bg, radius, region):
    """One image: regions first (a superpixel whose in-bounds clicks all carry one label), then the disks in click order
    (foreground clicks, then background clicks: pack_hints' order), the later click winning."""
    out = np.array(mask, dtype=np.uint8, copy=True)
    h, w = out.shape
    clicks = [(int(r), int(c), 1) for r, c in fg] + [(int(r), int(c), 0) for r, c in bg]
    clicks = [(r, c, l) for r, c, l in clicks if 0 <= r < h and 0 <= c < w]
    if region:
        labels = {}
        for r, c, l in clicks:
            labels.setdefault(int(seg[r, c]), set()).add(l)
        for s, ls in labels.items():
            if len(ls) == 1:
                out[seg == s] = ls.pop()
    yy, xx = np.mgrid[0:h, 0:w]
    for r, c, l in clicks:
        out[(yy - r) ** 2 + (xx - c) ** 2 <= radius * radius] = l
    return out


def disk_labels(h, w, fg, bg, radius):
    """(H,W) int: the label the disks alone paint at each pixel, -1 where none does."""
    lab = paint(np.full((h, w), 255, np.uint8), None, fg, bg, radius, False).astype(np.int32)
    lab[lab == 255] = -1
    return lab


def _apply(eng, masks, segs, per_image, radius, region, with_nodes=True):
    from gcn_grabcut.graph_builder import pack_hints
    b, h, w = masks.shape
    counts = [int(s.max()) + 1 for s in segs]
    node_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rows, ptr = pack_hints(per_image)
    hints, hint_ptr = eng.upload_hints(rows, ptr)
    m = eng.to_device(masks)
    seg = eng.to_device(segs.astype(np.int32))
    nptr = eng.to_device(node_ptr)
    table = torch.full((int(node_ptr[-1]), 3), -1.0, device=eng.device) if with_nodes else None
    eng.apply_hints(m, hints, hint_ptr, radius, region, seg, nptr, table)
    return m.cpu().numpy(), (table.cpu().numpy() if with_nodes else None), node_ptr


def _block_segments(rng, h, w):
    """A label map of rectangular blocks under a random permutation: labels 0..n-1, all present."""
    bh, bw = int(rng.integers(4, 9)), int(rng.integers(4, 11))
    ids = (np.arange(h)[:, None] // bh) * (w // bw + 1) + np.arange(w)[None, :] // bw
    _, inv = np.unique(ids, return_inverse=True)
    perm = rng.permutation(inv.max() + 1)
    return perm[inv.reshape(h, w)].astype(np.int32)


def _random_clicks(rng, h, w, n):
    pts = np.stack([rng.integers(-4, h + 4, n), rng.integers(-4, w + 4, n)], 1)
    pts[: min(n, 4)] = [(0, 0), (h - 1, w - 1), (0, w - 1), (h - 1, 0)][: min(n, 4)]   # the borders
    return [tuple(int(v) for v in p) for p in pts]


def _kernel_batch(seed=7, h=37, w=53):
    rng = np.random.default_rng(seed)
    masks = rng.integers(0, 4, (6, h, w)).astype(np.uint8)
    segs = np.stack([_block_segments(rng, h, w) for _ in range(6)])
    per_image = []
    for b in range(6):
        if b == 5:
            per_image.append(None)                                      # no clicks
            continue
        n = int(rng.integers(1, 41))
        pts = _random_clicks(rng, h, w, n)
        k = int(rng.integers(0, n + 1))
        fg, bg = pts[:k], pts[k:]
        if b == 0:                                                      # one superpixel clicked with both labels,
            fg, bg = fg + [(10, 10), (12, 12)], bg + [(10, 11), (11, 12)]   # overlapping disks of both labels
        per_image.append((fg, bg))
    return masks, segs, per_image


@pytest.mark.parametrize("region", [0, 1])
@pytest.mark.parametrize("radius", [0, 1, 7])
def test_apply_hints_matches_the_restatement(radius, region):
    from gcn_grabcut._engine import get_engine
    from gcn_grabcut.graph_builder import encode_user_hints
    eng = get_engine("cuda")
    masks, segs, per_image = _kernel_batch()
    got, table, node_ptr = _apply(eng, masks, segs, per_image, radius, region)
    for b in range(6):
        fg, bg = per_image[b] if per_image[b] is not None else ([], [])
        want = paint(masks[b], segs[b], fg, bg, radius, region)
        assert np.array_equal(got[b], want), (b, radius, region)
        assert np.array_equal(table[node_ptr[b]:node_ptr[b + 1]], encode_user_hints(segs[b], fg, bg)), b
    assert np.array_equal(got[5], masks[5])


@pytest.mark.parametrize("region", [0, 1])
def test_apply_hints_more_clicks_than_one_culling_pass(region):
    """300 clicks on one image with radius 9: some tiles see more than the 256 clicks one pass of the culled list holds."""
    from gcn_grabcut._engine import get_engine
    from gcn_grabcut.graph_builder import encode_user_hints
    eng = get_engine("cuda")
    rng = np.random.default_rng(3)
    h, w = 45, 70
    masks = rng.integers(0, 4, (2, h, w)).astype(np.uint8)
    segs = np.stack([_block_segments(rng, h, w) for _ in range(2)])
    pts = [(int(rng.integers(0, 12)), int(rng.integers(0, 20))) for _ in range(300)]
    per_image = [(pts[:170], pts[170:]), ([(20, 30)], [])]
    got, table, node_ptr = _apply(eng, masks, segs, per_image, 9, region)
    for b in range(2):
        fg, bg = per_image[b]
        assert np.array_equal(got[b], paint(masks[b], segs[b], fg, bg, 9, region)), b
        assert np.array_equal(table[node_ptr[b]:node_ptr[b + 1]], encode_user_hints(segs[b], fg, bg)), b


def test_apply_hints_argument_checks():
    from gcn_grabcut import _native
    from gcn_grabcut._engine import get_engine
    eng = get_engine("cuda")
    mask = torch.full((2, 9, 11), 3, dtype=torch.uint8, device=eng.device)
    hints, ptr = eng.upload_hints(np.array([[1, 1, 1]], np.int32), np.array([0, 1, 1], np.int32))
    with pytest.raises(_native.GGCError, match="INVALID_ARG"):
        eng.apply_hints(mask, hints, ptr, -1)
    for bad in ([0, 2, 1], [1, 1, 1]):                                  # decreasing; not starting at 0
        _, bad_ptr = eng.upload_hints(np.array([[1, 1, 1]] * 2, np.int32), np.array(bad, np.int32))
        with pytest.raises(_native.GGCError, match="INVALID_ARG"):
            eng.apply_hints(mask, hints, bad_ptr, 2)
    _, empty = eng.upload_hints(np.zeros((0, 3), np.int32), np.zeros(3, np.int32))
    eng.apply_hints(mask, None, empty, 2)                               # K == 0: a no-op
    assert bool((mask == 3).all())
    eng.apply_hints(mask, hints, ptr, 0)
    assert int(mask[0, 1, 1]) == 1 and int((mask != 3).sum()) == 1


# ---------------------------------------------------------------- pipeline

HINTED = (0, 5)


def _batch_hints(h, w):
    return [([(20, 30), (h - 1, w - 1)], [(3, 3), (21, 33), (-5, 2)]) if b == 0 else
            ([(h // 2, w // 2)], [(h // 2, w // 2 + 6), (0, w - 2)]) if b == 5 else None for b in range(8)]


@pytest.fixture(scope="module")
def hinted_runs():
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig
    from gcn_grabcut.synthetic import synthetic_batch
    model, sd = seeded_state_dict(32, 2, seed=5)
    pipe = GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=60), device="cuda")
    imgs = synthetic_batch(8, 64, 96, config_id=9)
    bgr = pipe._eng.to_device(imgs)
    hints = _batch_hints(64, 96)
    base = pipe.segment_batch_device(bgr, chunks=1)
    hinted = pipe.segment_batch_device(bgr, chunks=1, hints=hints, hint_radius=4)
    return pipe, imgs, bgr, hints, base, hinted


KEYS = ("binary_mask", "trimap", "segments", "probs", "gc_mask", "overlay", "rgba")


def test_pipeline_hints_leave_other_images_alone(hinted_runs):
    pipe, imgs, bgr, hints, base, hinted = hinted_runs
    g0, g1 = base["graphs"], hinted["graphs"]
    for b in range(8):
        if b in HINTED:
            continue
        for k in ("binary_mask", "trimap", "segments", "gc_mask", "overlay", "rgba"):
            assert torch.equal(base[k][b], hinted[k][b]), (b, k)
        n0, n1 = g0.node_ptr_host[b], g0.node_ptr_host[b + 1]
        assert torch.equal(base["probs"][n0:n1], hinted["probs"][n0:n1]), b
    assert torch.equal(base["probs"], hinted["probs"])                  # hard constraints do not touch the network
    assert torch.equal(g0.x, g1.x)


def test_pipeline_hints_are_hard_constraints_on_the_grabcut_trimap(hinted_runs, oracle):
    pipe, imgs, bgr, hints, base, hinted = hinted_runs
    for b in HINTED:
        fg, bg = hints[b]
        tri0 = base["trimap"][b].cpu().numpy()
        want = paint(tri0, None, fg, bg, 4, False)
        tri = hinted["trimap"][b].cpu().numpy()
        assert np.array_equal(tri, want), b
        assert not np.array_equal(tri, tri0), b
        binary, m, _, _, _ = oracle.grabcut(imgs[b], want, n_iter=pipe.gc_config.n_iter, mode=0, seed=pipe.gc_config.seed + b)
        assert np.array_equal(hinted["gc_mask"][b].cpu().numpy(), m), b
        assert np.array_equal(hinted["binary_mask"][b].cpu().numpy(), oracle.clean_mask(binary, 0.002)), b


def test_pipeline_hint_disks_survive_without_clean_up(hinted_runs):
    pipe, imgs, bgr, hints, base, hinted = hinted_runs
    out = pipe.segment_batch_device(bgr, chunks=1, hints=hints, hint_radius=4, min_area_ratio=0.0)
    for b in HINTED:
        lab = disk_labels(64, 96, *hints[b], 4)
        binm = out["binary_mask"][b].cpu().numpy()
        assert (lab == 1).any() and (lab == 0).any()
        assert (binm[lab == 1] == 1).all(), b
        assert (binm[lab == 0] == 0).all(), b


@pytest.mark.parametrize("region", [False, True])
def test_pipeline_hints_chunked_equals_one_chunk(hinted_runs, region):
    pipe, imgs, bgr, hints, base, hinted = hinted_runs
    one = hinted if not region else pipe.segment_batch_device(bgr, chunks=1, hints=hints, hint_radius=4, hint_region=True)
    four = pipe.segment_batch_device(bgr, chunks=4, hints=hints, hint_radius=4, hint_region=region)
    for k in KEYS:
        assert torch.equal(one[k], four[k]), k
    if region:                                                          # the region pass changed something
        assert not torch.equal(one["trimap"], hinted["trimap"])


def test_pipeline_packed_hints_equal_per_image_lists(hinted_runs):
    from gcn_grabcut.graph_builder import pack_hints
    pipe, imgs, bgr, hints, base, hinted = hinted_runs
    rows, ptr = pack_hints(hints)
    out = pipe.segment_batch_device(bgr, chunks=1, hints=(torch.from_numpy(rows), torch.from_numpy(ptr)), hint_radius=4)
    for k in KEYS:
        assert torch.equal(out[k], hinted[k]), k


def test_pipeline_hints_as_prior(hinted_runs):
    from gcn_grabcut.graph_builder import encode_user_hints
    pipe, imgs, bgr, hints, base, hinted = hinted_runs
    out = pipe.segment_batch_device(bgr, chunks=1, hints=hints, hint_radius=4, hints_as_prior=True)
    g = base["graphs"]
    x = g.x.clone()
    seg = base["segments"].cpu().numpy()
    for b in HINTED:
        n0, n1 = g.node_ptr_host[b], g.node_ptr_host[b + 1]
        x[n0:n1, 16:19] = torch.from_numpy(encode_user_hints(seg[b], *hints[b])).to(x.device)
    want = pipe._eng.predict_probs(pipe.model, replace(g, x=x))
    assert torch.equal(out["probs"], want)
    assert torch.equal(out["graphs"].x, x)
    assert not torch.equal(out["probs"], base["probs"])
    for b in range(8):                                                  # images without clicks: the automatic prior
        if b not in HINTED:
            n0, n1 = g.node_ptr_host[b], g.node_ptr_host[b + 1]
            assert torch.equal(out["probs"][n0:n1], base["probs"][n0:n1]), b


def test_segment_takes_clicks(hinted_runs):
    pipe, imgs, bgr, hints, base, hinted = hinted_runs
    fg, bg = hints[5]
    r = pipe.segment(imgs[5], fg_points=fg, bg_points=bg, hint_radius=4)
    one = pipe.segment_batch_device(bgr[5:6], hints=[hints[5]], hint_radius=4)
    assert np.array_equal(r.trimap, one["trimap"][0].cpu().numpy())
    assert np.array_equal(r.binary_mask, one["binary_mask"][0].cpu().numpy())
    plain = pipe.segment(imgs[5])
    assert np.array_equal(plain.trimap, pipe.segment_batch_device(bgr[5:6])["trimap"][0].cpu().numpy())
    assert np.array_equal(r.trimap, paint(plain.trimap, None, fg, bg, 4, False))


# ---------------------------------------------------------------- GrabCut.add_hints

def test_grabcut_add_hints_then_refine(oracle):
    from gcn_grabcut import GrabCut
    from gcn_grabcut.synthetic import synthetic_image
    img = synthetic_image(70, 90, 1234)
    gc = GrabCut(img, device="cuda")
    with pytest.raises(RuntimeError):
        gc.add_hints(fg_points=[(5, 5)])
    tri = np.full((70, 90), 2, np.uint8)
    tri[20:50, 25:65] = 3
    tri[30:40, 35:55] = 1
    tri[:4] = 0
    gc.run_with_trimap(tri)
    m0, bgd, fgd = gc.mask.copy(), gc._bgd.copy(), gc._fgd.copy()
    fg, bg = [(60, 10), (8, 80)], [(35, 45), (62, 14)]
    gc.add_hints(fg_points=fg, bg_points=bg, radius=3)
    painted = paint(m0, None, fg, bg, 3, False)
    assert np.array_equal(gc.mask, painted)
    assert gc.history[-1].tag == "hints"
    gc.refine(2)
    _, want, _, _, _ = oracle.grabcut(img, painted, n_iter=2, mode=2, seed=gc.config.seed, bgd=bgd, fgd=fgd)
    assert np.array_equal(gc.mask, want)
    lab = disk_labels(70, 90, fg, bg, 3)
    assert (gc.mask[lab == 1] == 1).all() and (gc.mask[lab == 0] == 0).all()


def test_grabcut_add_hints_sees_host_edits_of_the_mask():
    from gcn_grabcut import GrabCut
    from gcn_grabcut.synthetic import synthetic_image
    gc = GrabCut(synthetic_image(40, 50, 99), device="cuda")
    gc.run_with_bbox((10, 8, 30, 24))
    gc.mask[0, :] = 1                                                   # edited on the host, as before this API
    edited = gc.mask.copy()
    gc.add_hints(bg_points=[(20, 20)], radius=2)
    assert np.array_equal(gc.mask, paint(edited, None, [], [(20, 20)], 2, False))


# ---------------------------------------------------------------- CLI

def test_cli_clicks_are_scaled_and_kept(tmp_path):
    from PIL import Image
    from gcn_grabcut.synthetic import synthetic_image
    img = synthetic_image(300, 400, 4242)
    Image.fromarray(img[:, :, ::-1]).save(tmp_path / "x.png")
    model, sd = seeded_state_dict(32, 2, seed=8)
    torch.save({"model": sd, "epoch": 1}, tmp_path / "ckpt.pt")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--image", str(tmp_path / "x.png"), "--output", str(out),
                        "--checkpoint", str(tmp_path / "ckpt.pt"), "--superpixels", "100", "--max-size", "200",
                        "--min-area", "0", "--save", "mask", "--fg-point", "100,150", "--bg-point", "250,40",
                        "--fg-point", "290,390", "--hint-radius", "2"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    mask = np.asarray(Image.open(out / "x_mask.png"))
    assert mask.shape == (150, 200)                                     # the --max-size resize halved the image
    assert mask[50, 75] == 255 and mask[145, 195] == 255                # (100,150), (290,390) scaled by 1/2
    assert mask[125, 20] == 0                                           # (250,40)
    lab = disk_labels(150, 200, [(50, 75), (145, 195)], [(125, 20)], 2)
    assert (mask[lab == 1] == 255).all() and (mask[lab == 0] == 0).all()
