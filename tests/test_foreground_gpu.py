"""ggc_estimate_foreground on the MI355X: known pixels exact, a residual certificate recomputed in float64 on the host,
agreement with the restatement (tests/foreground_ref.py) on the premultiplied colours, bit-for-bit batch independence,
the quality margins settled in test_foreground_cpu.py, argument checks, the pipeline and the command line."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from foreground_ref import (ALPHA_SOURCES, alpha_input, pcg, premult_levels, quality_ratio, residual_norms,
                            scene_colours, snap, to_u8)
from matte_ref import alpha_matte_ref, edge_band
from test_foreground_cpu import AGREE_LEVELS, BAD_ARGS, DEFAULTS, QUALITY, SCENES

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F32 = lambda v: float(np.float32(v))                              # the entry takes eps_r, omega and tol as float32


def _stream():
    from gcn_grabcut import _native
    return _native.current_stream(0)


def _call(ctx, bgr, alpha, eps_r=5e-3, omega=1.0, max_iter=2000, tol=1e-6):
    """ggc_estimate_foreground on (B,H,W,3) uint8 / (B,H,W) float32 arrays -> dict of device tensors."""
    bgr = torch.as_tensor(np.ascontiguousarray(bgr)).cuda()
    alpha = torch.as_tensor(np.ascontiguousarray(alpha, np.float32)).cuda()
    b, h, w, _ = bgr.shape
    out = dict(foreground=torch.empty(b, h, w, 3, dtype=torch.uint8, device="cuda"),
               rgba=torch.empty(b, h, w, 4, dtype=torch.uint8, device="cuda"),
               raw_f=torch.empty(b, h, w, 3, dtype=torch.float64, device="cuda"),
               raw_b=torch.empty(b, h, w, 3, dtype=torch.float64, device="cuda"),
               iters=torch.empty(b, dtype=torch.int32, device="cuda"),
               rel=torch.empty(b, dtype=torch.float64, device="cuda"))
    ctx.call("ggc_estimate_foreground", _stream(), b, h, w, bgr.data_ptr(), alpha.data_ptr(), eps_r, omega, max_iter, tol,
             out["foreground"].data_ptr(), out["rgba"].data_ptr(), out["raw_f"].data_ptr(), out["raw_b"].data_ptr(),
             out["iters"].data_ptr(), out["rel"].data_ptr())
    torch.cuda.synchronize()
    return out


def _synthetic(h, w, seed):
    from gcn_grabcut.synthetic import synthetic_image
    return synthetic_image(h, w, seed, return_mask=True)


def _grabcut_case(h, w, seed):
    from gcn_grabcut import GrabCut
    img, _ = _synthetic(h, w, seed)
    mask = GrabCut(img).run_with_bbox((w // 5, h // 6, 3 * w // 5, 2 * h // 3)).astype(np.uint8)
    assert 0 < mask.sum() < mask.size
    return img, mask


def _scene_cases():
    for kind, seed in SCENES:
        img = scene_colours(kind, seed)[0]
        for source in ALPHA_SOURCES:
            yield f"{kind}{seed}-{source}", img, alpha_input(kind, seed, source)


def _cases():
    out = list(_scene_cases())
    img, mask = _grabcut_case(96, 128, 3)
    out.append(("grabcut3", img, alpha_matte_ref(img, mask, 4, 1e-4).astype(np.float32)))
    img, gt = _synthetic(53, 67, 9)
    out.append(("odd53x67", img, alpha_matte_ref(img, gt, 2, 1e-4).astype(np.float32)))
    return out


def test_known_pixels_exact_and_residual_certificate(gpu_ctx):
    eps_r, omega, max_iter, tol = 5e-3, 1.0, 2000, 1e-6
    for name, img, alpha in _cases():
        o = _call(gpu_ctx, img[None], alpha[None], eps_r, omega, max_iter, tol)
        s = snap(alpha)
        U = (s > 0) & (s < 1)
        assert U.any(), name
        fg, rgba = o["foreground"][0].cpu().numpy(), o["rgba"][0].cpu().numpy()
        raw_f, raw_b = o["raw_f"][0].cpu().numpy(), o["raw_b"][0].cpu().numpy()
        assert np.array_equal(fg[~U], img[~U]), name
        assert np.array_equal(raw_f[~U], img[~U] / 255.0) and np.array_equal(raw_b[~U], img[~U] / 255.0), name
        assert np.array_equal(fg[U], to_u8(raw_f)[U]) and np.array_equal(rgba[..., :3], fg), name
        assert np.array_equal(rgba[..., 3], to_u8(alpha.astype(np.float64))), name      # rgba_soft's byte of this alpha
        iters, rel = int(o["iters"][0]), float(o["rel"][0])
        assert 1 <= iters <= max_iter, (name, iters)
        res, res0 = residual_norms(img, s, F32(eps_r), F32(omega), raw_f, raw_b)
        print(f"{name}: |U| {U.sum()}, iterations {iters}, residual {res / res0:.3e} (reported {rel:.3e})")
        assert res <= 2.0 * tol * res0, (name, res / res0)
        assert abs(rel - res / res0) <= 0.1 * (res / res0), (name, rel, res / res0)
        assert rel <= tol, (name, rel)


def test_agrees_with_the_restatement_on_premultiplied_colours(gpu_ctx):
    d = DEFAULTS
    for name, img, alpha in _scene_cases():
        o = _call(gpu_ctx, img[None], alpha[None], d["eps_r"], d["omega"], d["max_iter"], d["tol"])
        s = snap(alpha)
        F, B, _, _ = pcg(img, s, d["eps_r"], d["omega"], 20000, 1e-12)
        gf, gb = premult_levels(s, o["raw_f"][0].cpu().numpy(), o["raw_b"][0].cpu().numpy())
        wf, wb = premult_levels(s, F, B)
        df, db = np.abs(gf - wf).max(), np.abs(gb - wb).max()
        print(f"{name}: iterations {int(o['iters'][0])}, premultiplied F {df:.3f} B {db:.3f} levels")
        assert df <= AGREE_LEVELS and db <= AGREE_LEVELS, (name, df, db)


def _mixed_batch(h=44, w=60):
    rng = np.random.default_rng(21)
    imgs = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(8)]
    alphas = [np.zeros((h, w), np.float32), np.ones((h, w), np.float32), np.full((h, w), 0.5, np.float32)]
    one = np.zeros((h, w), np.float32)
    one[h // 2, w // 3] = 0.3
    alphas.append(one)                                           # one fractional pixel
    alphas.append(rng.random((h, w)).astype(np.float32))         # noise
    imgs[5] = np.full((h, w, 3), 90, np.uint8)                   # flat colour under random alpha: F = B = I solves it
    alphas.append(rng.random((h, w)).astype(np.float32))
    blob = np.clip(1.5 - np.hypot(*np.mgrid[-h // 2:h - h // 2, -w // 2:w - w // 2]) / 8.0, 0, 1).astype(np.float32)
    alphas.append(blob)                                          # a soft blob inside tiles 1..2
    alphas.append(np.clip(rng.normal(0.5, 0.6, (h, w)), -0.5, 1.5).astype(np.float32))   # values beyond [0, 1]
    return np.stack(imgs), np.stack(alphas)


def test_batch_equals_single_image_calls_bit_for_bit(gpu_ctx):
    imgs, alphas = _mixed_batch()
    args = (5e-3, 1.0, 400, 1e-6)
    full = _call(gpu_ctx, imgs, alphas, *args)
    again = _call(gpu_ctx, imgs, alphas, *args)
    for k in full:
        assert torch.equal(full[k], again[k]), k
    for j in range(len(imgs)):
        one = _call(gpu_ctx, imgs[j:j + 1], alphas[j:j + 1], *args)
        for k in full:
            assert torch.equal(one[k][0], full[k][j]), (j, k)
    it = full["iters"].cpu().numpy()
    print("iterations", it.tolist(), "raw F range of the one-pixel image",
          float(full["raw_f"][3].min()), float(full["raw_f"][3].max()))
    assert it[0] == 0 and it[1] == 0 and it[5] == 0
    assert (it[[2, 3, 4, 6, 7]] >= 1).all() and (it <= 400).all()
    fg = full["foreground"].cpu().numpy()
    for j in (0, 1, 5):
        assert np.array_equal(fg[j], imgs[j]), j
    assert np.array_equal(full["rgba"].cpu().numpy()[..., 3], to_u8(alphas.astype(np.float64)))
    # the degenerate members against the restatement, where the problem is well posed (premultiplied colours)
    for j in (2, 3, 4, 6, 7):
        s = snap(alphas[j])
        F, B, n_it, _ = pcg(imgs[j], s, F32(args[0]), args[1], 20000, 1e-12)
        gf, gb = premult_levels(s, full["raw_f"][j].cpu().numpy(), full["raw_b"][j].cpu().numpy())
        wf, wb = premult_levels(s, F, B)
        print(f"image {j}: premultiplied F {np.abs(gf - wf).max():.3f} B {np.abs(gb - wb).max():.3f} levels")
        assert np.abs(gf - wf).max() <= AGREE_LEVELS and np.abs(gb - wb).max() <= AGREE_LEVELS, j


def test_nan_alpha_is_snapped_to_zero(gpu_ctx):
    imgs, alphas = _mixed_batch()
    a = alphas[6:7].copy()
    bad = a.copy()
    bad[0, 3, 5] = np.nan                                        # a pixel of the blob's surround (alpha 0)
    bad[0, 22, 30] = np.nan                                      # a pixel inside it
    clean = bad.copy()
    clean[np.isnan(clean)] = 0.0
    x, y = _call(gpu_ctx, imgs[6:7], bad), _call(gpu_ctx, imgs[6:7], clean)
    for k in x:
        assert torch.equal(x[k], y[k]), k
    assert torch.isfinite(x["raw_f"]).all() and int(x["rgba"][0, 22, 30, 3]) == 0


@pytest.mark.parametrize("source", ALPHA_SOURCES)
@pytest.mark.parametrize("kind,seed", SCENES)
def test_clean_cutout_beats_the_image_bytes(gpu_ctx, kind, seed, source):
    # margins settled on the restatement first (test_foreground_cpu.py::test_restatement_meets_the_quality_...)
    img, a_true, mask, fg_true, _ = scene_colours(kind, seed)
    alpha = alpha_input(kind, seed, source)
    d = DEFAULTS
    o = _call(gpu_ctx, img[None], alpha[None], d["eps_r"], d["omega"], d["max_iter"], d["tol"])
    ratio = quality_ratio(alpha, o["raw_f"][0].cpu().numpy(), img, a_true, fg_true, edge_band(mask, 8))
    print(f"{kind}{seed} {source}: iterations {int(o['iters'][0])}, ratio {ratio:.3f}")
    assert ratio <= QUALITY[source]


# ---------------------------------------------------------------- arguments
ENTRY_BAD = [(a, -1) for a in BAD_ARGS if float(a[2]) == int(a[2])]            # a fractional max_iter cannot reach the entry


@pytest.mark.parametrize("args,code", ENTRY_BAD)
def test_entry_refuses_bad_arguments(gpu_ctx, args, code):
    from gcn_grabcut import _native
    from gcn_grabcut._engine import get_engine
    imgs, alphas = _mixed_batch(10, 12)
    with pytest.raises(_native.GGCError) as e:
        _call(gpu_ctx, imgs[:1], alphas[:1], args[0], args[1], int(args[2]), args[3])
    assert e.value.code == code
    eng = get_engine("cuda")
    with pytest.raises(ValueError):
        eng.estimate_foreground(torch.as_tensor(imgs[:1]).cuda(), torch.as_tensor(alphas[:1]).cuda(), *args)


def test_entry_refuses_bad_shapes_and_a_call_without_outputs_and_accepts_an_empty_batch(gpu_ctx):
    from gcn_grabcut import _native
    from gcn_grabcut._engine import get_engine
    imgs, alphas = _mixed_batch(10, 12)
    bgr, a = torch.as_tensor(imgs[:1]).cuda(), torch.as_tensor(alphas[:1]).cuda()
    with pytest.raises(_native.GGCError) as e:
        gpu_ctx.call("ggc_estimate_foreground", _stream(), 1, 10, 12, bgr.data_ptr(), a.data_ptr(), 5e-3, 1.0, 10, 1e-6,
                     None, None, None, None, None, None)
    assert e.value.code == -1
    out = torch.empty(1, 10, 12, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(_native.GGCError) as e:
        gpu_ctx.call("ggc_estimate_foreground", _stream(), 1, 0, 12, bgr.data_ptr(), a.data_ptr(), 5e-3, 1.0, 10, 1e-6,
                     out.data_ptr(), None, None, None, None, None)
    assert e.value.code == -2
    with pytest.raises(_native.GGCError) as e:
        gpu_ctx.call("ggc_estimate_foreground", _stream(), 1, 10, 12, None, a.data_ptr(), 5e-3, 1.0, 10, 1e-6,
                     out.data_ptr(), None, None, None, None, None)
    assert e.value.code == -1
    gpu_ctx.call("ggc_estimate_foreground", _stream(), 0, 10, 12, None, None, 5e-3, 1.0, 10, 1e-6, out.data_ptr(), None,
                 None, None, None, None)
    eng = get_engine("cuda")
    with pytest.raises(ValueError):
        eng.estimate_foreground(bgr, a[:, :, :6], 5e-3, 1.0, 10, 1e-6)
    with pytest.raises(ValueError):
        eng.estimate_foreground(bgr, a.double(), 5e-3, 1.0, 10, 1e-6)


def test_public_estimate_foreground(gpu_ctx):
    from gcn_grabcut import estimate_foreground
    img, a_true, mask, fg_true, _ = scene_colours("strands", 0)
    alpha = alpha_input("strands", 0, "true")
    f, it, rel = estimate_foreground(img, alpha, return_info=True)
    assert f.dtype == np.uint8 and f.shape == (120, 160, 3) and 1 <= it <= 2000 and rel <= 1e-6
    assert np.array_equal(f, estimate_foreground(img, alpha.astype(np.float64)))
    s = snap(alpha)
    U = (s > 0) & (s < 1)
    assert np.array_equal(f[~U], img[~U])
    sel = U & (a_true > 0.1)
    before, after = np.abs(img - fg_true)[sel].mean(), np.abs(f - fg_true)[sel].mean()
    print(f"mean |colour - F*| on 0.1 < alpha* < 1: image {before:.1f} levels, foreground {after:.1f}")
    assert after <= 0.25 * before                                # the issue's table: 62-70 levels before, 3-9 after


# ---------------------------------------------------------------- pipeline and command line
@pytest.fixture(scope="module")
def pipe():
    from helpers import seeded_state_dict
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig
    model, _ = seeded_state_dict(64, 3, seed=4)
    return GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=100), device="cuda:0")


@pytest.mark.parametrize("kw", [dict(chunks=1, grabcut_lanes=1), dict(chunks=1, grabcut_lanes=4),
                                dict(chunks=2, grabcut_lanes=4)])
@pytest.mark.parametrize("kind", ["guided", "closed-form"])
def test_pipeline_foreground_leaves_every_other_output_unchanged(pipe, kw, kind):
    from gcn_grabcut import ClosedFormMatte, ForegroundColours
    from gcn_grabcut._engine import get_engine
    from gcn_grabcut.synthetic import synthetic_batch
    bgr = torch.as_tensor(synthetic_batch(32, 72, 96, config_id=8)).cuda()
    matte = True if kind == "guided" else ClosedFormMatte(radius=2, band=2)
    fgc = ForegroundColours(tol=1e-5)
    soft = pipe.segment_batch_device(bgr, matte=matte, **kw)
    clean = pipe.segment_batch_device(bgr, matte=matte, foreground=fgc, **kw)
    torch.cuda.synchronize()
    assert "foreground" not in soft and "rgba_clean" not in soft
    for k in ("binary_mask", "trimap", "overlay", "rgba", "gc_mask", "alpha", "rgba_soft"):
        assert torch.equal(soft[k], clean[k]), k
    eng = get_engine("cuda")
    want, want_rgba, iters, _ = eng.estimate_foreground(bgr, clean["alpha"], *fgc.args(), want_rgba=True)
    assert torch.equal(clean["foreground"], want) and torch.equal(clean["rgba_clean"], want_rgba)
    assert torch.equal(clean["rgba_clean"][..., :3], clean["foreground"])
    # the alpha byte is taken from the float32 alpha; rgba_soft's from the float64 value before that rounding, so the
    # two can differ by one level where 255 alpha + 0.5 lies within a float32 ulp of an integer
    diff = (clean["rgba_clean"][..., 3].int() - clean["rgba_soft"][..., 3].int()).abs()
    print(f"{kind} {kw}: iterations {iters.min().item()}..{iters.max().item()}, alpha bytes that differ {int((diff > 0).sum())}")
    assert int(diff.max()) <= 1
    frac = (clean["rgba_soft"][..., 3] > 0) & (clean["rgba_soft"][..., 3] < 255)
    assert frac.any() and (clean["foreground"][frac] != bgr[frac]).any()
    true_fg = clean["foreground"] == bgr
    assert true_fg[~frac & (diff == 0)].all()                    # the image's bytes wherever alpha is 0 or 255


def test_segment_segment_bbox_and_segment_batch_fill_the_foreground(pipe, tmp_path):
    from gcn_grabcut import ClosedFormMatte, ForegroundColours, estimate_foreground
    img, _ = _synthetic(80, 100, 41)
    r = pipe.segment(img, matte=True, foreground=True)
    assert r.foreground.shape == (80, 100, 3) and r.rgba_clean.shape == (80, 100, 4)
    assert np.array_equal(r.foreground, estimate_foreground(img, r.alpha))
    assert np.array_equal(r.rgba_clean[..., :3], r.foreground)
    plain = pipe.segment(img, matte=True)
    assert plain.foreground is None and plain.rgba_clean is None and np.array_equal(plain.rgba_soft, r.rgba_soft)
    rb = pipe.segment_bbox(img, (20, 15, 60, 50), matte=ClosedFormMatte(band=2), foreground=ForegroundColours(omega=0.5))
    assert np.array_equal(rb.foreground, estimate_foreground(img, rb.alpha, omega=0.5))
    assert np.array_equal(rb.rgba_clean[..., :3], rb.foreground)
    rg = pipe.segment_bbox(img, (20, 15, 60, 50), matte=True, foreground=True)
    assert np.array_equal(rg.foreground, estimate_foreground(img, rg.alpha))
    res = pipe.segment_batch([img, img[::-1].copy()], matte=ClosedFormMatte(), foreground=True)
    assert all(np.array_equal(x.foreground, estimate_foreground(x.image, x.alpha)) for x in res)
    with pytest.raises(ValueError, match="matte"):
        pipe.segment(img, foreground=True)
    with pytest.raises(ValueError, match="matte"):
        pipe.segment_batch_device(torch.as_tensor(img[None]).cuda(), foreground=True)
    big = np.repeat(np.repeat(img, 2, 0), 2, 1)
    with pytest.raises(ValueError, match="full"):
        pipe.segment(img, matte=True, foreground=True, full_image=big)
    with pytest.raises(ValueError, match="full"):
        pipe.segment_batch_device(torch.as_tensor(img[None]).cuda(), matte=True, foreground=True,
                                  full_bgr=torch.as_tensor(big[None]).cuda())
    with pytest.raises(ValueError):
        pipe.segment(img, matte=True, foreground=ForegroundColours(tol=2.0))
    from PIL import Image
    r.save(str(tmp_path / "out"))
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out_cutout_clean.png"))[..., [2, 1, 0, 3]], r.rgba_clean)
    plain.save(str(tmp_path / "plain"))
    assert not (tmp_path / "plain_cutout_clean.png").exists()


def test_inference_cli_writes_the_clean_cutout_only_with_decontaminate(tmp_path):
    from PIL import Image
    from helpers import seeded_state_dict
    from gcn_grabcut.synthetic import synthetic_image
    in_dir = tmp_path / "in"
    in_dir.mkdir()
    images = [synthetic_image(72, 96, 600 + k) for k in range(2)]
    for k, im in enumerate(images):
        Image.fromarray(im[:, :, ::-1]).save(in_dir / f"im{k}.png")
    _, sd = seeded_state_dict(64, 3, seed=5)
    torch.save({"model": sd, "epoch": 1}, tmp_path / "ckpt.pt")

    def run(out, *extra):
        r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--input", str(in_dir), "--output", str(out),
                            "--checkpoint", str(tmp_path / "ckpt.pt"), "--superpixels", "100", "--max-size", "0",
                            "--save", "mask", "alpha", "cutout", *extra], cwd=tmp_path, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return {p.name: p.read_bytes() for p in out.iterdir()}

    plain = run(tmp_path / "plain")
    clean = run(tmp_path / "clean", "--decontaminate")
    names = sorted(f"im{k}_{s}.png" for k in range(2) for s in ("mask", "alpha", "cutout"))
    assert sorted(plain) == names and sorted(clean) == names
    changed = 0
    for k in range(2):
        for s in ("mask", "alpha"):
            assert plain[f"im{k}_{s}.png"] == clean[f"im{k}_{s}.png"], (k, s)
        a = np.asarray(Image.open(tmp_path / "plain" / f"im{k}_alpha.png")).astype(np.int64)
        cut0 = np.asarray(Image.open(tmp_path / "plain" / f"im{k}_cutout.png"))
        cut1 = np.asarray(Image.open(tmp_path / "clean" / f"im{k}_cutout.png"))
        assert cut1.shape == cut0.shape == (72, 96, 4)
        assert np.array_equal(cut0[..., :3], images[k][:, :, ::-1])          # without the flag: the image's own bytes
        assert np.abs(cut1[..., 3].astype(np.int64) - a).max() <= 1 and np.abs(cut0[..., 3].astype(np.int64) - a).max() <= 1
        solid = (cut1[..., 3] == 0) | (cut1[..., 3] == 255)
        assert np.array_equal(cut1[..., :3][solid], cut0[..., :3][solid])
        changed += int((cut1[..., :3] != cut0[..., :3]).any(-1).sum())
    assert changed > 0
