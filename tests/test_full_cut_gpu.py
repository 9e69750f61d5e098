"""The full-resolution banded cut on the MI355X: ggc_lift_labels against the numpy restatement (tests/full_cut_ref.py)
bit for bit, its band against ggc_closed_form_band on the device, batch independence and refusals; cut_mask_full against
the chain of CPU oracle entries bit for bit, the quality totals test_full_cut_cpu.py records, and the pipeline option
and command line that use it."""
import functools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import full_cut_ref as fc
from test_full_cut_cpu import CUT_TOTALS, GUIDED_TOTALS

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SENTINEL = 77


def _stream():
    from gcn_grabcut import _native
    return _native.current_stream(0)


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype)).cuda()


def _lift(ctx, masks, full, band, want=(True, True)):
    """ggc_lift_labels on a (B,H,W) array -> (labels, mask_full) numpy arrays (None where not wanted)."""
    m = _dev(masks, np.uint8)
    b, h, w = m.shape
    out = [torch.full((b, *full), SENTINEL, dtype=torch.uint8, device="cuda") if k else None for k in want]
    ctx.call("ggc_lift_labels", _stream(), b, h, w, m.data_ptr(), full[0], full[1], band,
             *[None if t is None else t.data_ptr() for t in out])
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def _masks(shape, seed):
    """(4,H,W) uint8: noise with the bytes 1, 255 and 7 as foreground, a disk, an empty and a full mask."""
    rng = np.random.default_rng(seed)
    h, w = shape
    noise = rng.choice(np.array([0, 0, 0, 1, 255, 7], np.uint8), size=shape)
    yy, xx = np.mgrid[0:h, 0:w]
    disk = (((yy - 0.45 * h) / (0.3 * h)) ** 2 + ((xx - 0.55 * w) / (0.35 * w)) ** 2 <= 1.0).astype(np.uint8) * 255
    return np.stack([noise, disk, np.zeros(shape, np.uint8), np.full(shape, 7, np.uint8)])


LIFT_SHAPES = [((7, 9), (7, 9)), ((13, 17), (37, 50)), ((24, 32), (96, 128)), ((30, 40), (111, 148)), ((9, 70), (20, 300))]


# ---------------------------------------------------------------- 1-4: the entry
@pytest.mark.parametrize("shape,full", LIFT_SHAPES)
@pytest.mark.parametrize("band", [0, 1, 5, 64])
def test_lift_labels_equals_the_restatement(gpu_ctx, shape, full, band):
    masks = _masks(shape, shape[0] * 1000 + full[1] + band)
    want = [fc.lift_labels(m, full, band) for m in masks]
    labels, lifted = _lift(gpu_ctx, masks, full, band)
    only_labels, none = _lift(gpu_ctx, masks, full, band, (True, False))
    none2, only_mask = _lift(gpu_ctx, masks, full, band, (False, True))
    assert none is None and none2 is None
    for i, (wl, wm) in enumerate(want):
        assert np.array_equal(labels[i], wl), (i, int((labels[i] != wl).sum()))
        assert np.array_equal(lifted[i], wm), i
        assert np.array_equal(only_labels[i], wl) and np.array_equal(only_mask[i], wm), i
    assert (labels[2] == 0).all() and (labels[3] == 1).all()                  # empty and full: no band
    if shape == full:
        assert np.array_equal(lifted, (masks != 0).astype(np.uint8))          # every weight is 0


@pytest.mark.parametrize("shape,full", LIFT_SHAPES[1:])
@pytest.mark.parametrize("band", [0, 5, 64])
def test_band_is_the_closed_form_band_of_the_lifted_mask(gpu_ctx, shape, full, band):
    from gcn_grabcut._engine import get_engine
    eng = get_engine("cuda")
    labels, lifted = eng.lift_labels(_dev(_masks(shape, 5)), full, band, want_labels=True, want_mask=True)
    trimap = eng.closed_form_band(lifted, band)
    assert torch.equal(labels >= 2, trimap == 128)
    assert torch.equal(labels & 1, lifted)


def test_every_image_is_independent_of_its_batch(gpu_ctx):
    shape, full, band = (30, 40), (111, 148), 5
    m = _masks(shape, 9)
    batch = np.stack([m[0], m[2], m[1]])                                     # a trivial image in the middle
    labels, lifted = _lift(gpu_ctx, batch, full, band)
    for i in range(3):
        one = _lift(gpu_ctx, batch[i:i + 1], full, band)
        assert np.array_equal(labels[i], one[0][0]) and np.array_equal(lifted[i], one[1][0]), i


def test_refusals_and_the_no_op(gpu_ctx):
    from gcn_grabcut import _native
    m = _dev(_masks((12, 14), 1))
    out = torch.full((4, 24, 28), SENTINEL, dtype=torch.uint8, device="cuda")

    def call(b, h1, w1, band, labels, mask):
        gpu_ctx.call("ggc_lift_labels", _stream(), b, 12, 14, m.data_ptr(), h1, w1, band, labels, mask)

    for args, code in (((4, 11, 28, 1, out.data_ptr(), None), "GGC_E_SHAPE"), ((4, 24, 13, 1, out.data_ptr(), None), "GGC_E_SHAPE"),
                       ((4, 24, 32769, 1, out.data_ptr(), None), "GGC_E_SHAPE"),
                       ((4, 24, 28, -1, out.data_ptr(), None), "GGC_E_INVALID_ARG"),
                       ((4, 24, 28, 65, out.data_ptr(), None), "GGC_E_INVALID_ARG"),
                       ((4, 24, 28, 1, None, None), "GGC_E_INVALID_ARG")):
        with pytest.raises(_native.GGCError) as e:
            call(*args)
        assert _native.ERROR_NAMES.get(e.value.code) == code, args
    call(0, 24, 28, 1, out.data_ptr(), None)                                  # B == 0 does nothing
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


# ---------------------------------------------------------------- 5-6: the cut
@functools.lru_cache(maxsize=None)
def _scene(seed, size=(240, 320, 4)):
    h1, w1, k = size
    full, truth, _ = fc.scene(h1, w1, seed, k)
    return full, truth, fc.working_masks(truth, k)


@functools.lru_cache(maxsize=None)
def _device_cut(seed, which, n_iter=1, color_space="rgb"):
    from gcn_grabcut import cut_mask_full
    full, _, masks = _scene(seed)
    return cut_mask_full(masks[which], full, n_iter=n_iter, color_space=color_space)


@pytest.mark.parametrize("seed", [30000, 30001, 30002])
def test_cut_mask_full_equals_the_oracle_chain(oracle, seed):
    full, _, masks = _scene(seed)
    for which in (0, 1):
        for n_iter in (1, 2):
            for cs in ("rgb", "lab"):
                got = _device_cut(seed, which, n_iter, cs)
                want = fc.chain(masks[which], full, None, n_iter, 0, cs)
                assert got.shape == full.shape[:2] and got.dtype == np.uint8
                assert np.array_equal(got, want), (which, n_iter, cs, int((got != want).sum()))


def test_cut_mask_full_labels_seed_and_trivial_masks(oracle):
    from gcn_grabcut import cut_mask_full, lift_labels
    full, _, masks = _scene(30001)
    got, labels = cut_mask_full(masks[1], full, band=3, seed=5, keep_largest=True, return_labels=True)
    want, want_labels = fc.chain(masks[1], full, 3, 1, 5, "rgb", 0.002, True, return_labels=True)
    assert np.array_equal(labels, want_labels) and np.array_equal(got, want)
    assert np.array_equal(lift_labels(masks[1], full.shape[:2], 3), want_labels)
    assert np.array_equal(lift_labels(masks[1], full.shape[:2]), fc.lift_labels(masks[1], full.shape[:2], 6)[0])
    for mask in (np.zeros_like(masks[0]), np.ones_like(masks[0])):           # no band: GrabCut's degenerate guard
        lifted = fc.lift_labels(mask, full.shape[:2], 6)[1]
        assert np.array_equal(cut_mask_full(mask, full), lifted)
        assert np.array_equal(fc.chain(mask, full), lifted)


def test_cut_of_a_batch_at_600x800_equals_the_oracle_chain(oracle):
    """Two images of 600x800 from 150x200: the max-flow runs over many tiles whose pixels are mostly definite."""
    from gcn_grabcut._engine import get_engine
    eng = get_engine("cuda")
    scenes = [_scene(30000 + j, (600, 800, 4)) for j in range(2)]
    masks = np.stack([s[2][j] for j, s in enumerate(scenes)])               # image 0 good, image 1 shifted
    fulls = np.stack([s[0] for s in scenes])
    band = fc.default_band(masks.shape[1:], fulls.shape[1:3])
    assert band == 6
    got = eng.cut_mask_full(_dev(masks), _dev(fulls), band, seed=3).cpu().numpy()
    for j in range(2):
        want = fc.chain(masks[j], fulls[j], band, 1, 3 + j)
        assert np.array_equal(got[j], want), (j, int((got[j] != want).sum()))


def test_device_totals_are_the_recorded_ones():
    """The quality claim on the device: the summed wrong pixels of the six scenes are those of the CPU oracle chain."""
    totals = [0, 0]
    for seed in fc.STUDY_SEEDS:
        truth = _scene(seed)[1]
        for which in (0, 1):
            totals[which] += fc.wrong(_device_cut(seed, which), truth)
    print(f"device totals {totals}")
    assert tuple(totals) == CUT_TOTALS
    assert all(10 * totals[j] <= GUIDED_TOTALS[j] for j in (0, 1))


# ---------------------------------------------------------------- 7: the pipeline
@pytest.fixture(scope="module")
def pipe():
    from helpers import seeded_state_dict
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig
    model, _ = seeded_state_dict(64, 3, seed=4)
    return GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=100), device="cuda:0")


def _pair(seed, h=72, w=96, k=3):
    from gcn_grabcut.synthetic import synthetic_image
    from upsample_ref import resize_bgr
    img = synthetic_image(h, w, seed)
    return img, resize_bgr(img, h * k, w * k)


def test_segment_fills_the_full_mask_from_the_cut(pipe):
    from gcn_grabcut import ClosedFormMatte, FullCut, cut_mask_full
    img, full = _pair(41)
    seed, cs = pipe.gc_config.seed, pipe.gc_config.color_space
    plain = pipe.segment(img, matte=True, full_image=full)
    r = pipe.segment(img, matte=True, full_image=full, full_cut=True)
    for k in ("binary_mask", "trimap", "segments", "overlay", "rgba", "alpha", "rgba_soft"):
        assert np.array_equal(getattr(r, k), getattr(plain, k)), k
    assert np.array_equal(r.full.alpha, plain.full.alpha) and np.array_equal(r.full.rgba_soft, plain.full.rgba_soft)
    want = cut_mask_full(r.binary_mask, full, seed=seed, color_space=cs)
    assert r.full.binary_mask.shape == full.shape[:2] and np.array_equal(r.full.binary_mask, want)
    assert np.array_equal(r.full.rgba[..., 3], 255 * r.full.binary_mask) and np.array_equal(r.full.rgba[..., :3], full)
    assert r.full.overlay.shape == full.shape
    bare = pipe.segment(img, full_image=full, full_cut=True)                 # without a matte no upsample runs at all
    assert bare.full.alpha is None and np.array_equal(bare.full.binary_mask, want)
    tuned = pipe.segment(img, full_image=full, full_cut=FullCut(band=2, n_iter=2))
    assert np.array_equal(tuned.full.binary_mask, cut_mask_full(tuned.binary_mask, full, band=2, n_iter=2, seed=seed, color_space=cs))
    rb = pipe.segment_bbox(img, (20, 15, 60, 50), full_image=full, full_cut=True)
    assert np.array_equal(rb.full.binary_mask, cut_mask_full(rb.binary_mask, full, seed=seed, color_space=cs))
    assert np.array_equal(rb.full.rgba[..., 3], 255 * rb.full.binary_mask)
    with pytest.raises(ValueError, match="full image"):
        pipe.segment(img, full_cut=True)
    with pytest.raises(ValueError, match="closed_form_matte"):
        pipe.segment(img, full_image=full, full_cut=True, matte=ClosedFormMatte(full_resolution=True))


def test_segment_batch_with_the_cut_does_not_depend_on_the_schedule(pipe, monkeypatch):
    from gcn_grabcut import cut_mask_full
    from gcn_grabcut import pipeline as P
    pairs = [_pair(50 + j) for j in range(4)]
    imgs, fulls = [p[0] for p in pairs], [p[1] for p in pairs]
    base = pipe.segment_batch(imgs, full_images=fulls, full_cut=True)
    chunked = pipe.segment_batch(imgs, full_images=fulls, full_cut=True, chunks=2, grabcut_lanes=2)
    monkeypatch.setattr(P, "FULL_CUT_PIXELS", 1)                             # one image per ggc_grabcut call
    split = pipe.segment_batch(imgs, full_images=fulls, full_cut=True)
    seed = pipe.gc_config.seed
    for b, x in enumerate(base):
        for other in (chunked[b], split[b]):
            assert np.array_equal(other.binary_mask, x.binary_mask)
            for k in ("binary_mask", "overlay", "rgba"):
                assert np.array_equal(getattr(other.full, k), getattr(x.full, k)), (b, k)
        assert np.array_equal(x.full.binary_mask, cut_mask_full(x.binary_mask, fulls[b], seed=seed + b)), b


# ---------------------------------------------------------------- 8: the command line
def test_inference_cli_writes_the_cut_mask(tmp_path):
    from PIL import Image
    from helpers import seeded_state_dict
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig, cut_mask_full
    from inference import read_bgr
    in_dir = tmp_path / "in"
    in_dir.mkdir()
    for k in range(2):
        Image.fromarray(_pair(600 + k)[1][:, :, ::-1]).save(in_dir / f"im{k}.png")       # 216 x 288
    model, sd = seeded_state_dict(64, 3, seed=5)
    torch.save({"model": sd, "epoch": 1}, tmp_path / "ckpt.pt")
    out = tmp_path / "cut"
    base = [sys.executable, str(ROOT / "inference.py"), "--input", str(in_dir), "--output", str(out),
            "--checkpoint", str(tmp_path / "ckpt.pt"), "--superpixels", "100", "--max-size", "96"]
    r = subprocess.run(base + ["--full-res", "--full-mask", "cut", "--save", "mask", "cutout"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(p.name for p in out.iterdir()) == sorted(f"im{k}_{s}.png" for k in range(2) for s in ("mask", "cutout"))
    pipe = GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=100), device="cuda:0")
    pairs = [read_bgr(in_dir / f"im{k}.png", 96, keep_original=True) for k in range(2)]
    work = pipe.segment_batch([p[0] for p in pairs])
    for k in range(2):
        mask = np.asarray(Image.open(out / f"im{k}_mask.png"))
        assert mask.shape == (216, 288) and Image.open(out / f"im{k}_cutout.png").size == (288, 216)
        assert np.array_equal(mask, 255 * cut_mask_full(work[k].binary_mask, pairs[k][1], seed=k))
    r = subprocess.run(base + ["--full-mask", "cut"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--full-res" in r.stderr
    r = subprocess.run(base + ["--full-res", "--full-mask", "cut", "--matte-method", "closed-form-full", "--save", "alpha"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "closed-form-full" in r.stderr
