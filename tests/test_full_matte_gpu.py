"""The full-resolution closed-form matte on the MI355X: ggc_lift_trimap against the float64 restatement
(tests/full_matte_ref.py) bit for bit, ggc_trimap_matte_warm against ggc_trimap_matte (same bits from 0.5), against the
restatement and a residual certificate recomputed on the host, the quality and the saved iterations the restatement
shows at 480x640, and the pipeline and command lines that chain them.  The bounds are settled on the restatement in
test_full_matte_cpu.py."""
import functools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import full_matte_ref as fm
import trimap_matte_ref as tm
from closed_form_ref import strand_scene
from test_full_matte_cpu import LIFT_SHAPES, QUALITY_SLACK, RATIO, TAU, _random_case

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KEYS = ("alpha", "rgba", "raw", "iters", "rel")
R, EPS, BAND, MAX_ITER, TOL = fm.CF


def _stream():
    from gcn_grabcut import _native
    return _native.current_stream(0)


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype)).cuda()


def _lift(ctx, trimap, alpha, full, grow=0, want=(True, True)):
    """ggc_lift_trimap on (B,H,W) arrays -> (trimap_full, alpha0_full) numpy arrays (None where not wanted)."""
    t, a = _dev(trimap), _dev(alpha, np.float32)
    b, h, w = t.shape
    t_full = torch.full((b, *full), 77, dtype=torch.uint8, device="cuda") if want[0] else None
    a_full = torch.full((b, *full), -7.0, device="cuda") if want[1] else None
    ctx.call("ggc_lift_trimap", _stream(), b, h, w, t.data_ptr(), a.data_ptr(), full[0], full[1], grow,
             None if t_full is None else t_full.data_ptr(), None if a_full is None else a_full.data_ptr())
    torch.cuda.synchronize()
    return (None if t_full is None else t_full.cpu().numpy()), (None if a_full is None else a_full.cpu().numpy())


def _solve(ctx, entry, bgr, trimap, alpha0, r=R, eps=EPS, max_iter=fm.FULL_MAX_ITER, tol=TOL):
    """ggc_trimap_matte / ggc_trimap_matte_warm on (B,H,W,3) / (B,H,W) arrays -> dict of device tensors."""
    bgr, trimap = _dev(bgr), _dev(trimap)
    a0 = None if alpha0 is None else _dev(alpha0, np.float32)
    b, h, w, _ = bgr.shape
    out = dict(alpha=torch.empty(b, h, w, device="cuda"), rgba=torch.empty(b, h, w, 4, dtype=torch.uint8, device="cuda"),
               raw=torch.empty(b, h, w, dtype=torch.float64, device="cuda"),
               iters=torch.empty(b, dtype=torch.int32, device="cuda"), rel=torch.empty(b, dtype=torch.float64, device="cuda"))
    ctx.call(entry, _stream(), b, h, w, bgr.data_ptr(), trimap.data_ptr(), r, eps, max_iter, tol,
             None if a0 is None else a0.data_ptr(), *[out[k].data_ptr() for k in KEYS])
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------- the lift
GPU_LIFT_SHAPES = LIFT_SHAPES + [((30, 41), (30, 41)), ((30, 41), (60, 82)), ((30, 41), (120, 164)), ((30, 42), (100, 140)),
                                 ((33, 47), (101, 259))]


@pytest.mark.parametrize("grow", [0, 1, 5])
@pytest.mark.parametrize("shape,full", GPU_LIFT_SHAPES)
def test_lift_equals_the_restatement_bit_for_bit(gpu_ctx, shape, full, grow):
    cases = [_random_case(*shape, seed=s) for s in (1, 2, 3)]
    t, a = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    got_t, got_a = _lift(gpu_ctx, t, a, full, grow)
    for j in range(3):
        want_t, want_a = fm.lift(t[j], a[j], full, grow)
        assert np.array_equal(got_t[j], want_t), (j, np.argwhere(got_t[j] != want_t)[:5])
        assert np.array_equal(got_a[j], want_a), (j, np.abs(got_a[j].astype(np.float64) - want_a).max())
    # either output alone is the same output
    only_t, none_a = _lift(gpu_ctx, t, a, full, grow, want=(True, False))
    none_t, only_a = _lift(gpu_ctx, t, a, full, grow, want=(False, True))
    assert none_a is None and none_t is None and np.array_equal(only_t, got_t) and np.array_equal(only_a, got_a)


def test_lift_identity_and_batch_independence(gpu_ctx):
    cases = [_random_case(37, 53, seed=s) for s in range(5)]
    t, a = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    a[1] = np.inf
    a[2, 3, 4] = -np.inf
    got_t, got_a = _lift(gpu_ctx, t, a, (37, 53), 0)
    assert np.array_equal(got_t, np.where(t == 255, 255, np.where(t == 0, 0, 128)))
    assert np.array_equal(got_a, np.clip(np.where(np.isnan(a), 0.0, a), 0.0, 1.0).astype(np.float32))
    for full, grow in (((37, 53), 4), ((80, 190), 0), ((123, 177), 7)):
        whole_t, whole_a = _lift(gpu_ctx, t, a, full, grow)
        for j in range(5):
            one_t, one_a = _lift(gpu_ctx, t[j:j + 1], a[j:j + 1], full, grow)
            assert np.array_equal(one_t[0], whole_t[j]) and np.array_equal(one_a[0], whole_a[j])


def test_lift_refusals(gpu_ctx):
    from gcn_grabcut._native import GGCError
    t = torch.zeros(2, 10, 12, dtype=torch.uint8, device="cuda")
    a = torch.zeros(2, 10, 12, device="cuda")
    tf = torch.zeros(2, 20, 24, dtype=torch.uint8, device="cuda")
    af = torch.zeros(2, 20, 24, device="cuda")

    def call(b=2, h=10, w=12, t_p=t.data_ptr(), a_p=a.data_ptr(), h1=20, w1=24, grow=0, tf_p=tf.data_ptr(), af_p=af.data_ptr()):
        gpu_ctx.call("ggc_lift_trimap", _stream(), b, h, w, t_p, a_p, h1, w1, grow, tf_p, af_p)

    for kw, code in ((dict(h1=9), -2), (dict(w1=11), -2), (dict(h1=32769), -2), (dict(b=65536), -2), (dict(b=-1), -2),
                     (dict(h=0), -2), (dict(grow=-1), -1), (dict(grow=65), -1), (dict(tf_p=None, af_p=None), -1),
                     (dict(t_p=None), -1), (dict(a_p=None), -1)):
        with pytest.raises(GGCError) as e:
            call(**kw)
        assert e.value.code == code, (kw, e.value.code)
    call(b=0, t_p=None, a_p=None)                       # B == 0 does nothing
    call(t_p=None, tf_p=None)                           # an input is only read for its output
    call(a_p=None, af_p=None)
    torch.cuda.synchronize()


def test_band_entry_is_the_band_the_solver_used(gpu_ctx):
    """ggc_closed_form_band against the restatement's band, and through the solver itself: ggc_trimap_matte on it from
    the mask gives ggc_closed_form_matte's bits."""
    from gcn_grabcut._engine import get_engine
    eng = get_engine("cuda")
    scenes = [strand_scene(120, 160, seed=s) for s in (0, 1)]
    imgs, masks = np.stack([s[0] for s in scenes]), np.stack([s[2] for s in scenes])
    masks[1][masks[1] > 0] = 200                        # any nonzero byte is foreground
    for band in (0, 1, 3, 9):
        got = eng.closed_form_band(_dev(masks), band)
        assert np.array_equal(got.cpu().numpy(), np.stack([tm.trimap_from_mask(m, band) for m in masks]))
        want = eng.closed_form_matte(_dev(imgs), _dev(masks), R, EPS, band, MAX_ITER, TOL)
        again = eng.trimap_matte(_dev(imgs), got, R, EPS, MAX_ITER, TOL, alpha0=_dev(masks > 0, np.float32))
        for x, y in zip(want, again):
            assert torch.equal(x, y), band


# ---------------------------------------------------------------- the warm solver
@functools.lru_cache(maxsize=None)
def _case(i):
    return fm.warm_case(*fm.WARM_CASES[i])


@functools.lru_cache(maxsize=None)
def _exact(i):
    full, t_full, a0 = _case(i)
    x, _, rel = fm.pcg_warm(full, t_full, R, EPS, 20000, 1e-12, a0)
    assert rel <= 1e-12
    return x


def test_warm_from_one_half_is_the_cold_entry_bit_for_bit(gpu_ctx):
    for i in (0, 2):
        full, t_full, _ = _case(i)
        imgs, tris = np.stack([full, full[::-1]]), np.stack([t_full, t_full[::-1]])
        half = np.where((tris != 0) & (tris != 255), 0.5, np.random.default_rng(i).uniform(-3, 3, tris.shape))
        for max_iter, tol in ((fm.FULL_MAX_ITER, TOL), (9, 1e-9)):
            cold = _solve(gpu_ctx, "ggc_trimap_matte", imgs, tris, None, max_iter=max_iter, tol=tol)
            warm = _solve(gpu_ctx, "ggc_trimap_matte_warm", imgs, tris, half, max_iter=max_iter, tol=tol)
            assert int(cold["iters"].min()) > 0
            for k in KEYS:
                assert torch.equal(warm[k], cold[k]), (i, k, max_iter)


@pytest.mark.parametrize("i", range(len(fm.WARM_CASES)))
def test_warm_agrees_with_the_restatement_and_certifies_its_residual(gpu_ctx, i):
    """raw within TAU of the warm restatement solved to 1e-12.  TAU = 0.0294 is twice 0.0147, the largest
    |pcg_warm(tol 1e-4) - pcg_warm(tol 1e-12)| of the restatement over exactly these cases (tools/full_matte_study.py
    --tau; the worst is the 120x160 scene from 30x40 with grow 2), doubled because the device sums in another order and
    may stop an iteration earlier or later."""
    full, t_full, a0 = _case(i)
    o = _solve(gpu_ctx, "ggc_trimap_matte_warm", full[None], t_full[None], a0[None])
    raw, alpha = o["raw"][0].cpu().numpy(), o["alpha"][0].cpu().numpy()
    F, G, U = tm.regions(t_full)
    assert np.array_equal(raw[F], np.ones(F.sum())) and np.array_equal(raw[G], np.zeros(G.sum()))
    assert np.array_equal(alpha, np.clip(raw, 0.0, 1.0).astype(np.float32))
    err = float(np.abs(raw - _exact(i)).max())
    iters, rel = int(o["iters"][0]), float(o["rel"][0])
    res, ref = fm.residual_norms(full, t_full, raw, R, EPS)
    _, it_ref, _ = fm.pcg_warm(full, t_full, R, EPS, fm.FULL_MAX_ITER, TOL, a0)
    print(f"{fm.WARM_CASES[i]}: iters {iters} (restatement {it_ref}) rel {rel:.3e} recomputed {res / ref:.3e} err {err:.4f}")
    assert err <= TAU, err
    assert 1 <= iters <= fm.FULL_MAX_ITER and (rel <= TOL or iters == fm.FULL_MAX_ITER), (iters, rel)
    assert abs(rel - res / ref) <= 1e-6 * (res / ref), (rel, res / ref)


def test_warm_stops_on_its_start_or_at_max_iter(gpu_ctx):
    full, t_full, a0 = _case(0)
    done = _solve(gpu_ctx, "ggc_trimap_matte_warm", full[None], t_full[None], a0[None])
    # the solved alpha as the start: within tol already (clamping it moves the residual, so test at a looser tol)
    start = done["alpha"].cpu().numpy()
    res, ref = fm.residual_norms(full, t_full, tm.start_image(t_full, start[0]), R, EPS)
    again = _solve(gpu_ctx, "ggc_trimap_matte_warm", full[None], t_full[None], start, tol=float(res / ref) * 1.01)
    assert int(again["iters"][0]) == 0
    assert float(again["rel"][0]) == pytest.approx(res / ref, rel=1e-6)
    assert np.array_equal(again["raw"][0].cpu().numpy(), tm.start_image(t_full, start[0]))
    # the cold entry, which measures against its own start, iterates from there
    cold = _solve(gpu_ctx, "ggc_trimap_matte", full[None], t_full[None], start, tol=float(res / ref) * 1.01)
    assert int(cold["iters"][0]) > 0
    capped = _solve(gpu_ctx, "ggc_trimap_matte_warm", full[None], t_full[None], a0[None], max_iter=5)
    assert int(capped["iters"][0]) == 5 and float(capped["rel"][0]) > TOL


def test_warm_batch_independence_with_trivial_images(gpu_ctx):
    (f0, t0, a0), (f1, t1, a1) = _case(0), _case(1)
    imgs = np.stack([f0, f1, f0, f1])
    tris = np.stack([np.full_like(t0, 255), t1, t0, np.full_like(t1, 128)])
    starts = np.stack([a0, a1, a0, np.full_like(a1, 0.3)])
    whole = _solve(gpu_ctx, "ggc_trimap_matte_warm", imgs, tris, starts)
    assert whole["iters"].tolist()[0] == 0 == whole["iters"].tolist()[3]
    assert whole["rel"].tolist()[0] == 0.0 == whole["rel"].tolist()[3]
    assert np.array_equal(whole["raw"][0].cpu().numpy(), np.ones_like(a0, np.float64))
    assert np.array_equal(whole["raw"][3].cpu().numpy(), np.full_like(a1, 0.3).astype(np.float64))
    assert min(whole["iters"].tolist()[1:3]) > 0
    for j in range(4):
        one = _solve(gpu_ctx, "ggc_trimap_matte_warm", imgs[j:j + 1], tris[j:j + 1], starts[j:j + 1])
        for k in KEYS:
            assert torch.equal(one[k][0], whole[k][j]), (j, k)


def test_warm_refusals(gpu_ctx):
    from gcn_grabcut._native import GGCError
    from gcn_grabcut._engine import get_engine
    full, t_full, a0 = _case(3)
    with pytest.raises(GGCError) as e:
        _solve(gpu_ctx, "ggc_trimap_matte_warm", full[None], t_full[None], None)
    assert e.value.code == -1
    with pytest.raises(GGCError) as e:
        _solve(gpu_ctx, "ggc_trimap_matte_warm", full[None], t_full[None], a0[None], r=9)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        get_engine("cuda").trimap_matte(_dev(full[None]), _dev(t_full[None]), R, EPS, 10, TOL, warm=True)


# ---------------------------------------------------------------- quality and iterations, against the restatement's
@pytest.mark.parametrize("seed", [0, 1])
def test_full_size_solve_quality_and_saved_iterations(gpu_ctx, seed):
    """Whole-image SAD at 480x640 from the 120x160 working size: closed_form_matte_full / the upsampled hard mask within
    QUALITY_SLACK of the restatement's ratio (0.4483 and 0.4808, tools/full_matte_study.py --quality), below
    upsample_mask's alpha, and the warm solve in strictly fewer iterations than the cold one on the same lifted trimap."""
    from gcn_grabcut import (closed_form_matte, closed_form_matte_full, lift_trimap, trimap_matte, trimap_matte_warm,
                             upsample_mask)
    from gcn_grabcut.pipeline import nearest_upsample
    from gcn_grabcut._engine import get_engine
    full, at, work, mask = fm.full_scene(480, 640, 4, seed)
    a, it, rel = closed_form_matte_full(work, mask, full, return_info=True)
    assert a.shape == (480, 640) and a.dtype == np.float32 and np.array_equal(a, closed_form_matte_full(work, mask, full))
    s_full, s_mask = fm.sad(a, at), fm.sad(nearest_upsample(mask, 480, 640), at)
    s_up = fm.sad(upsample_mask(work, mask, full, 8, 1e-4)[0], at)
    # the same lifted trimap through the public pieces, cold
    band = get_engine("cuda").closed_form_band(_dev(mask[None]), BAND)[0].cpu().numpy()
    t_full, a0_full = lift_trimap(band, closed_form_matte(work, mask), (480, 640))
    b, it_cold, rel_cold = trimap_matte(full, t_full, max_iter=fm.FULL_MAX_ITER, return_info=True)
    c, it_warm, _ = trimap_matte_warm(full, t_full, a0_full, max_iter=fm.FULL_MAX_ITER, return_info=True)
    print(f"seed {seed}: SAD full {s_full:.1f} mask {s_mask:.1f} upsample_mask {s_up:.1f} ratio {s_full / s_mask:.4f} "
          f"(restatement {RATIO[seed]}); iterations warm {it} cold {it_cold}; max |warm - cold| {np.abs(a - b).max():.4f}")
    assert np.array_equal(c, a) and it_warm == it
    assert rel <= TOL and rel_cold <= TOL and it < fm.FULL_MAX_ITER
    assert s_full / s_mask <= RATIO[seed] + QUALITY_SLACK
    assert s_full < s_up
    assert it < it_cold


def test_trimap_matte_full_and_the_matte_cli(gpu_ctx, tmp_path):
    from PIL import Image
    from gcn_grabcut import lift_trimap, trimap_matte, trimap_matte_full, trimap_matte_warm
    full, at, work, _ = fm.full_scene(240, 320, 2, 3)
    t = tm.trimap_from_alpha(fm.box_down(at, 2), 1)
    a, it, rel = trimap_matte_full(work, t, full, return_info=True)
    t_full, a0_full = lift_trimap(t, trimap_matte(work, t), (240, 320))
    want = trimap_matte_warm(full, t_full, a0_full, max_iter=fm.FULL_MAX_ITER)
    assert np.array_equal(a, want) and 0 < it < fm.FULL_MAX_ITER and rel <= TOL
    grown = trimap_matte_full(work, t, full, grow=3)
    assert not np.array_equal(grown, a)
    Image.fromarray(work[:, :, ::-1]).save(tmp_path / "w.png")
    Image.fromarray(t).save(tmp_path / "t.png")
    Image.fromarray(full[:, :, ::-1]).save(tmp_path / "f.png")
    r = subprocess.run([sys.executable, str(ROOT / "matte.py"), "--image", str(tmp_path / "w.png"), "--trimap",
                        str(tmp_path / "t.png"), "--full-image", str(tmp_path / "f.png"), "--output", str(tmp_path / "out"),
                        "--save", "alpha", "cutout"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    alpha = np.asarray(Image.open(tmp_path / "out" / "w_alpha.png"))
    assert alpha.shape == (240, 320)
    assert np.array_equal(alpha, np.floor(a.astype(np.float64) * 255.0 + 0.5).astype(np.uint8))
    assert Image.open(tmp_path / "out" / "w_cutout.png").size == (320, 240)


# ---------------------------------------------------------------- pipeline and command line
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


def test_segment_fills_the_full_resolution_closed_form_matte(pipe):
    from gcn_grabcut import ClosedFormMatte, closed_form_matte_full
    img, full = _pair(41)
    on = ClosedFormMatte(full_resolution=True)
    r = pipe.segment(img, matte=on, full_image=full)
    plain = pipe.segment(img, matte=ClosedFormMatte())
    for k in ("binary_mask", "trimap", "segments", "overlay", "rgba", "alpha", "rgba_soft"):
        assert np.array_equal(getattr(r, k), getattr(plain, k)), k
    want = closed_form_matte_full(img, r.binary_mask, full)
    assert r.full.alpha.shape == full.shape[:2] and np.array_equal(r.full.alpha, want)
    assert np.array_equal(r.full.binary_mask, (want >= 0.5).astype(np.uint8))
    assert np.array_equal(r.full.rgba_soft[..., :3], full)
    assert np.abs(r.full.rgba_soft[..., 3].astype(np.int64) - np.floor(want.astype(np.float64) * 255.0 + 0.5)).max() <= 1
    assert np.array_equal(r.full.rgba[..., 3], r.full.binary_mask * 255) and r.full.overlay.shape == full.shape
    grown = pipe.segment(img, matte=ClosedFormMatte(full_resolution=True, grow=2, band=2), full_image=full)
    assert np.array_equal(grown.full.alpha, closed_form_matte_full(img, grown.binary_mask, full, band=2, grow=2))
    rb = pipe.segment_bbox(img, (20, 15, 60, 50), matte=on, full_image=full)
    assert np.array_equal(rb.full.alpha, closed_form_matte_full(img, rb.binary_mask, full))
    assert np.array_equal(rb.full.binary_mask, (rb.full.alpha >= 0.5).astype(np.uint8))
    with pytest.raises(ValueError, match="full"):
        pipe.segment(img, matte=ClosedFormMatte(), full_image=full)
    with pytest.raises(ValueError):
        pipe.segment(img, matte=on)


@pytest.mark.parametrize("kw", [dict(), dict(chunks=2, grabcut_lanes=2)])
def test_segment_batch_equals_the_singles(pipe, kw):
    from gcn_grabcut import ClosedFormMatte
    pairs = [_pair(50 + j) for j in range(4)]
    on = ClosedFormMatte(full_resolution=True)
    res = pipe.segment_batch([p[0] for p in pairs], matte=on, full_images=[p[1] for p in pairs], **kw)
    for (img, full), x in zip(pairs, res):
        one = pipe.segment(img, matte=on, full_image=full)
        for k in ("binary_mask", "alpha", "rgba_soft"):
            assert np.array_equal(getattr(x, k), getattr(one, k)), k
        for k in ("alpha", "binary_mask", "rgba_soft", "overlay", "rgba"):
            assert np.array_equal(getattr(x.full, k), getattr(one.full, k)), k


def test_inference_cli_writes_the_full_size_alpha(tmp_path):
    from PIL import Image
    from helpers import seeded_state_dict
    in_dir = tmp_path / "in"
    in_dir.mkdir()
    for k in range(2):
        Image.fromarray(_pair(600 + k)[1][:, :, ::-1]).save(in_dir / f"im{k}.png")       # 216 x 288
    _, sd = seeded_state_dict(64, 3, seed=5)
    torch.save({"model": sd, "epoch": 1}, tmp_path / "ckpt.pt")
    out = tmp_path / "cf"
    r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--input", str(in_dir), "--output", str(out),
                        "--checkpoint", str(tmp_path / "ckpt.pt"), "--superpixels", "100", "--max-size", "96", "--full-res",
                        "--matte-method", "closed-form-full", "--save", "mask", "alpha", "cutout"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(p.name for p in out.iterdir()) == sorted(f"im{k}_{s}.png" for k in range(2)
                                                           for s in ("mask", "alpha", "cutout"))
    for k in range(2):
        alpha, mask = Image.open(out / f"im{k}_alpha.png"), Image.open(out / f"im{k}_mask.png")
        cut = Image.open(out / f"im{k}_cutout.png")
        assert alpha.mode == "L" and alpha.size == (288, 216) == mask.size and cut.mode == "RGBA" and cut.size == (288, 216)
        a = np.asarray(alpha).astype(np.int64)
        assert np.abs(np.asarray(cut)[..., 3].astype(np.int64) - a).max() <= 1
        assert np.array_equal(np.asarray(mask) > 0, a >= 128)
