"""ggc_matte_errors on the MI355X against the restatement (tests/matte_eval_ref.py): the four integer sums and the level
map equal, GRAD within 1e-9 (1 + ref) of the raw sum, bit-for-bit batch independence and repeatability, the entry's
refusals, the host API and the command line.

The GRAD bound: each filtered value is at most 81 products of magnitude <= 1 (error about 1e-14), so a term
(m_a - m_g)^2 is off by about 2 |m_a - m_g| 1e-14 and, by Cauchy-Schwarz, the sum by about 2e-14 sqrt(n GRAD)
<= 2e-11 sqrt(GRAD) for n <= 1e6, plus n 2^-53 relative for the accumulation: far inside 1e-9 (1 + GRAD)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from closed_form_ref import strand_scene
from matte_eval_ref import (blocky_levels, conventional, fading_levels, matte_errors_ref, random_levels, tie_case, to_levels)
from matte_ref import alpha_matte_ref, soft_disk_scene

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
INTS = ("n", "sad", "sse", "conn")
GRAD_RTOL = 1e-9
SHAPES = [(1, 1), (1, 37), (41, 1), (7, 130), (300, 400), (600, 800)]
SCENES = {"disk0": lambda: soft_disk_scene(seed=0), "disk1": lambda: soft_disk_scene(seed=1),
          "strands0": lambda: strand_scene(seed=0)}


def _stream():
    from gcn_grabcut import _native
    return _native.current_stream(0)


def _call(ctx, a, g, region=None, want_grad=True, want_levels=True):
    """ggc_matte_errors on (B,H,W) uint8 arrays -> (sums (B,4) int64, grad (B,) float64 or None, levels or None)."""
    a = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    g = torch.as_tensor(np.ascontiguousarray(g)).cuda()
    r = None if region is None else torch.as_tensor(np.ascontiguousarray(region)).cuda()
    b, h, w = a.shape
    sums = torch.full((b, 4), -1, dtype=torch.int64, device="cuda")
    grad = torch.full((b,), -1.0, dtype=torch.float64, device="cuda") if want_grad else None
    lev = torch.full((b, h, w), 99, dtype=torch.uint8, device="cuda") if want_levels else None
    ctx.call("ggc_matte_errors", _stream(), b, h, w, a.data_ptr(), g.data_ptr(), None if r is None else r.data_ptr(),
             sums.data_ptr(), None if grad is None else grad.data_ptr(), None if lev is None else lev.data_ptr())
    torch.cuda.synchronize()
    return (sums.cpu().numpy(), None if grad is None else grad.cpu().numpy(), None if lev is None else lev.cpu().numpy())


def _scene_cases():
    """The three scenes x {hard mask, the restatement's guided matte, the device's closed-form matte}, 120 x 160."""
    from gcn_grabcut import closed_form_matte
    out = []
    for name, make in SCENES.items():
        img, alpha, mask = make()
        gt = to_levels(alpha)
        out.append((f"{name}-hard", (mask * 255).astype(np.uint8), gt))
        out.append((f"{name}-guided", to_levels(alpha_matte_ref(img, mask, 4, 1e-4)), gt))
        out.append((f"{name}-closed", to_levels(closed_form_matte(img, mask)), gt))
    return out


def _small_cases():
    """Every 120 x 160 case: the scenes, uniform-random levels, images whose S_k is empty from some k on, blocks."""
    rng = np.random.default_rng(160)
    out = _scene_cases()
    out.append(("random", random_levels(rng, 120, 160), random_levels(rng, 120, 160)))
    out.append(("random-self", *(2 * [random_levels(rng, 120, 160)])))
    out.append(("fading", fading_levels(120, 160, 120), fading_levels(120, 160, 200)))
    out.append(("fading-dim", fading_levels(120, 160, 20), fading_levels(120, 160, 255)))      # S_k empty for every k
    out.append(("blocky", blocky_levels(rng, 120, 160, 5), blocky_levels(rng, 120, 160, 5)))
    return out


def _shape_cases():
    rng = np.random.default_rng(37)
    out = []
    for h, w in SHAPES:
        out.append((f"random{h}x{w}", random_levels(rng, h, w), random_levels(rng, h, w)))
        out.append((f"fading{h}x{w}", fading_levels(h, w, 130), fading_levels(h, w, 255)))
        out.append((f"blocky{h}x{w}", blocky_levels(rng, h, w), blocky_levels(rng, h, w)))
    a, g = tie_case()
    out.append(("tie", a, g))
    return out


def _check(name, got, want):
    sums, grad, lev = got
    print(f"{name}: n {want['n']} SAD {want['sad']} SSE {want['sse']} CONN {want['conn']} | device {sums.tolist()}"
          + ("" if grad is None else f" | GRAD ref {want['grad']:.17g} device {grad:.17g} "
                                     f"rel {abs(grad - want['grad']) / (1.0 + want['grad']):.2e}"))
    if lev is not None:
        assert np.array_equal(lev, want["levels"]), (name, int((lev != want["levels"]).sum()))
    assert sums.tolist() == [want[k] for k in INTS], (name, sums.tolist(), [want[k] for k in INTS])
    if grad is not None:
        assert abs(grad - want["grad"]) <= GRAD_RTOL * (1.0 + want["grad"]), (name, grad, want["grad"])


def _check_all_variants(ctx, name, a, g):
    rng = np.random.default_rng(len(name) + a.size)
    region = (rng.random(a.shape) < 0.4).astype(np.uint8) * rng.integers(1, 256, a.shape).astype(np.uint8)
    for tag, reg in (("whole", None), ("region", region)):
        want = matte_errors_ref(a, g, reg)
        r = None if reg is None else reg[None]
        sums, grad, lev = _call(ctx, a[None], g[None], r)
        _check(f"{name}/{tag}", (sums[0], grad[0], lev[0]), want)
        s2, g2, l2 = _call(ctx, a[None], g[None], r, want_levels=False)
        assert l2 is None and np.array_equal(s2, sums) and g2.tobytes() == grad.tobytes(), (name, tag)
        s3, g3, l3 = _call(ctx, a[None], g[None], r, want_grad=False)
        assert g3 is None and np.array_equal(s3, sums) and np.array_equal(l3, lev), (name, tag)
        s4, _, _ = _call(ctx, a[None], g[None], r, want_grad=False, want_levels=False)
        assert np.array_equal(s4, sums), (name, tag)


def test_sums_levels_and_grad_match_the_restatement_on_scenes_and_hard_cases(gpu_ctx):
    for name, a, g in _small_cases():
        _check_all_variants(gpu_ctx, name, a, g)


def test_sums_levels_and_grad_match_the_restatement_on_every_shape(gpu_ctx):
    for name, a, g in _shape_cases():
        _check_all_variants(gpu_ctx, name, a, g)


def test_hand_case_on_the_device(gpu_ctx):
    a, g = tie_case()
    sums, grad, lev = _call(gpu_ctx, a[None], g[None])
    assert sums[0].tolist() == [45, 408, 41616, 4080]
    assert (lev[0, 1:3, 1:3] == 10).all() and lev[0].sum() == 40


def test_mixed_batch_equals_single_calls_bit_for_bit_and_repeats(gpu_ctx):
    cases = _small_cases()
    a = np.stack([c[1] for c in cases] + [np.zeros((120, 160), np.uint8), np.full((120, 160), 255, np.uint8)])
    g = np.stack([c[2] for c in cases] + [np.zeros((120, 160), np.uint8), np.full((120, 160), 255, np.uint8)])
    rng = np.random.default_rng(6)
    region = (rng.random(a.shape) < 0.5).astype(np.uint8)
    for reg in (None, region):
        sums, grad, lev = _call(gpu_ctx, a, g, reg)
        again = _call(gpu_ctx, a, g, reg)
        assert np.array_equal(again[0], sums) and again[1].tobytes() == grad.tobytes() and np.array_equal(again[2], lev)
        for i in range(len(a)):
            s1, g1, l1 = _call(gpu_ctx, a[i:i + 1], g[i:i + 1], None if reg is None else reg[i:i + 1])
            assert np.array_equal(s1[0], sums[i]), i
            assert g1.view(np.uint64)[0] == grad.view(np.uint64)[i], (i, g1[0], grad[i])
            assert np.array_equal(l1[0], lev[i]), i
        if reg is None:
            assert sums[-2].tolist() == [19200, 0, 0, 0] and sums[-1].tolist() == [19200, 0, 0, 0]
            assert grad[-2] == 0.0 and grad[-1] == 0.0 and (lev[-2] == 0).all() and (lev[-1] == 10).all()


SCHEDULE_SCRIPT = """
import hashlib, sys
import numpy as np, torch
sys.path[:0] = [r'{root}', r'{root}/src', r'{root}/tests']
from gcn_grabcut._engine import get_engine
from matte_eval_ref import blocky_levels, random_levels
rng = np.random.default_rng(12)
a = np.stack([random_levels(rng, 90, 130), blocky_levels(rng, 90, 130, 4)])
g = np.stack([random_levels(rng, 90, 130), blocky_levels(rng, 90, 130, 4)])
eng = get_engine('cuda')
sums, grad, lev = eng.matte_errors(eng.to_device(a), eng.to_device(g), want_levels=True)
print('RESULT', sums.cpu().tolist(), grad.cpu().numpy().tobytes().hex(), hashlib.sha256(lev.cpu().numpy().tobytes()).hexdigest())
"""


def test_every_labelling_schedule_gives_the_same_result(gpu_ctx, tmp_path):
    """GGC_MATTE_EVAL_LEVELS is read once per process: one child per value, each under its own time limit."""
    import os
    rng = np.random.default_rng(12)
    a = np.stack([random_levels(rng, 90, 130), blocky_levels(rng, 90, 130, 4)])
    g = np.stack([random_levels(rng, 90, 130), blocky_levels(rng, 90, 130, 4)])
    want = [[matte_errors_ref(a[i], g[i])[k] for k in INTS] for i in range(2)]
    script = tmp_path / "schedule.py"
    script.write_text(SCHEDULE_SCRIPT.format(root=ROOT))
    seen = set()
    for levels in ("", "1", "2", "5", "10"):
        env = dict(os.environ)
        env.pop("GGC_MATTE_EVAL_LEVELS", None)
        if levels:
            env["GGC_MATTE_EVAL_LEVELS"] = levels
        r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (levels, r.stderr[-2000:])
        line = next(x for x in r.stdout.splitlines() if x.startswith("RESULT"))
        assert line.startswith(f"RESULT {want}"), (levels, line[:200], want)
        seen.add(line)
    assert len(seen) == 1


def test_entry_refusals(gpu_ctx):
    from gcn_grabcut._native import GGCError
    z = torch.zeros(4, 4, dtype=torch.uint8, device="cuda")
    sums = torch.full((1, 4), 7, dtype=torch.int64, device="cuda")
    p, s = z.data_ptr(), sums.data_ptr()

    def code(b, h, w, pred, gt, out):
        with pytest.raises(GGCError) as e:
            gpu_ctx.call("ggc_matte_errors", _stream(), b, h, w, pred, gt, None, out, None, None)
        return e.value.code

    for b, h, w in [(65536, 4, 4), (1, 0, 4), (1, 4, 0), (1, 32769, 1), (1, 1, 32769), (-1, 4, 4)]:
        assert code(b, h, w, p, p, s) == -2, (b, h, w)                   # GGC_E_SHAPE
    for pred, gt, out in [(None, p, s), (p, None, s), (p, p, None)]:
        assert code(1, 4, 4, pred, gt, out) == -1                        # GGC_E_INVALID_ARG
    gpu_ctx.call("ggc_matte_errors", _stream(), 0, 4, 4, p, p, None, s, None, None)          # B == 0 does nothing
    torch.cuda.synchronize()
    assert sums.cpu().tolist() == [[7, 7, 7, 7]]


def test_engine_refuses_bad_tensors_before_the_entry(gpu_ctx):
    from gcn_grabcut._engine import get_engine
    eng = get_engine("cuda")
    z = torch.zeros(1, 4, 5, dtype=torch.uint8, device="cuda")
    for bad in [(z, z[:, :, :4]), (z, z.float()), (z[0], z[0])]:
        with pytest.raises(ValueError):
            eng.matte_errors(*bad)
    with pytest.raises(ValueError):
        eng.matte_errors(z, z, region=z[:, :3])


# ---------------------------------------------------------------- host API and command line
def test_evaluate_matte_single_stack_uint8_and_float_agree():
    from gcn_grabcut import MatteMetrics, evaluate_matte, evaluate_matte_batch
    img, alpha, mask = soft_disk_scene(seed=0)
    gt = to_levels(alpha)
    pred_f = alpha_matte_ref(img, mask, 4, 1e-4)
    pred = to_levels(pred_f)
    want = conventional(matte_errors_ref(pred, gt))
    m = evaluate_matte(pred, gt)
    assert isinstance(m, MatteMetrics) and m.n_pixels == want["n_pixels"]
    assert (m.sad, m.mse, m.conn) == (want["sad"], want["mse"], want["conn"])
    assert abs(m.grad - want["grad"]) <= GRAD_RTOL * (1e-3 + want["grad"])
    assert evaluate_matte(pred_f, alpha) == m and evaluate_matte(pred_f, gt) == m and evaluate_matte(pred, alpha) == m
    region = np.abs(np.hypot(*np.mgrid[-59.5:60, -79.5:80]) - 40.0) < 6
    wr = conventional(matte_errors_ref(pred, gt, region))
    mr = evaluate_matte(pred, gt, region)
    assert (mr.n_pixels, mr.sad, mr.mse, mr.conn) == (wr["n_pixels"], wr["sad"], wr["mse"], wr["conn"])
    hard = (mask * 255).astype(np.uint8)
    stack = evaluate_matte(np.stack([pred, hard]), np.stack([gt, gt]))
    assert isinstance(stack, list) and stack[0] == m and stack[1] == evaluate_matte(hard, gt)
    small = tie_case()
    res = evaluate_matte_batch([dict(alpha=pred, gt_alpha=gt), dict(alpha=small[0], gt_alpha=small[1]),
                                dict(alpha=hard, gt_alpha=alpha), dict(alpha=pred, gt_alpha=gt, region=region)])
    assert res["n"] == 4 and res["metrics"] == [m, evaluate_matte(*small), stack[1], mr]
    for k in ("sad", "mse", "grad", "conn"):
        assert res[f"mean_{k}"] == float(np.mean([getattr(x, k) for x in res["metrics"]]))


def test_result_scores_its_own_matte():
    from helpers import seeded_state_dict
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig, evaluate_matte
    from gcn_grabcut.synthetic import synthetic_image
    model, _ = seeded_state_dict(64, 3, seed=4)
    pipe = GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=100), device="cuda:0")
    img, gt = synthetic_image(80, 100, 41, return_mask=True)
    r = pipe.segment(img, matte=True)
    gt_alpha = (gt != 0).astype(np.float64)
    m = r.evaluate_matte_against(gt_alpha)
    assert m == evaluate_matte(r.alpha, gt_alpha) and m.n_pixels == 8000
    want = conventional(matte_errors_ref(to_levels(r.alpha), to_levels(gt_alpha)))
    assert (m.sad, m.mse, m.conn) == (want["sad"], want["mse"], want["conn"])
    region = np.zeros((80, 100), np.uint8)
    region[20:60] = 1
    assert r.evaluate_matte_against(gt_alpha, region).n_pixels == 4000
    with pytest.raises(ValueError, match="matte"):
        pipe.segment(img).evaluate_matte_against(gt_alpha)


def test_cli_scores_saved_mattes_and_mattes_made_from_masks(tmp_path):
    from PIL import Image
    from gcn_grabcut import alpha_matte, closed_form_matte, evaluate_matte
    scenes = {name: make() for name, make in SCENES.items()}
    for sub in ("images", "masks", "alphas", "pred", "trimaps"):
        (tmp_path / sub).mkdir()
    truth, region, guided = {}, {}, {}
    for name, (img, alpha, mask) in scenes.items():
        truth[name] = to_levels(alpha)
        guided[name] = to_levels(alpha_matte_ref(img, mask, 4, 1e-4))
        tri = np.where(truth[name] == 0, 0, np.where(truth[name] == 255, 255, 128)).astype(np.uint8)
        region[name] = (tri == 128)
        Image.fromarray(img[:, :, ::-1]).save(tmp_path / "images" / f"{name}.png")
        Image.fromarray(mask * 255).save(tmp_path / "masks" / f"{name}.png")
        Image.fromarray(truth[name]).save(tmp_path / "alphas" / f"{name}.png")
        Image.fromarray(guided[name]).save(tmp_path / "pred" / f"{name}.png")
        Image.fromarray(tri).save(tmp_path / "trimaps" / f"{name}.png")
    small = tie_case()                                                   # a second shape: a second batch
    Image.fromarray(small[0]).save(tmp_path / "pred" / "tie.png")
    Image.fromarray(small[1]).save(tmp_path / "alphas" / "tie.png")
    Image.fromarray(np.full((5, 9), 128, np.uint8)).save(tmp_path / "trimaps" / "tie.png")

    def run(out, *argv):
        r = subprocess.run([sys.executable, str(ROOT / "evaluate_matte.py"), "--alphas", str(tmp_path / "alphas"),
                            "--json", str(out), *argv], cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "SAD" in r.stdout and "mean" in r.stdout
        with open(out) as f:
            return json.load(f)

    def same(doc, want):
        assert [d["name"] for d in doc["images"]] == sorted(want)
        for d in doc["images"]:
            assert {k: d[k] for k in ("sad", "mse", "grad", "conn", "n_pixels")} == want[d["name"]].as_dict(), d["name"]
        for k in ("sad", "mse", "grad", "conn"):
            assert doc["mean"][k] == float(np.mean([getattr(want[n], k) for n in sorted(want)]))

    want = {n: evaluate_matte(guided[n], truth[n]) for n in scenes}
    want["tie"] = evaluate_matte(*small)
    same(run(tmp_path / "a.json", "--pred", str(tmp_path / "pred")), want)
    want = {n: evaluate_matte(guided[n], truth[n], region[n]) for n in scenes}
    want["tie"] = evaluate_matte(*small)
    same(run(tmp_path / "b.json", "--pred", str(tmp_path / "pred"), "--trimaps", str(tmp_path / "trimaps")), want)
    from_masks = ["--images", str(tmp_path / "images"), "--masks", str(tmp_path / "masks")]
    want = {n: evaluate_matte(alpha_matte(s[0], s[2], 3, 1e-3), truth[n]) for n, s in scenes.items()}
    same(run(tmp_path / "c.json", *from_masks, "--method", "guided", "--matte-radius", "3", "--matte-eps", "1e-3"), want)
    want = {n: evaluate_matte(closed_form_matte(s[0], s[2], band=2), truth[n], region[n]) for n, s in scenes.items()}
    same(run(tmp_path / "d.json", *from_masks, "--method", "closed-form", "--cf-band", "2", "--trimaps",
             str(tmp_path / "trimaps")), want)
    want = {n: evaluate_matte((s[2] * 255).astype(np.uint8), truth[n]) for n, s in scenes.items()}
    same(run(tmp_path / "e.json", *from_masks, "--method", "mask"), want)
