"""experiment helper: ggc_matte_errors on batch 256 of 300x400 and batch 16 of 600x800.  pred = the guided matte
(defaults) of synthetic images' GrabCut masks, gt = the closed-form matte (defaults) of the same masks: two realistic soft
mattes of one object that differ along its edge.  Time per call from events over REPS (5) calls, with and without the
gradient filter; the bytes model of DESIGN.md 5.15; and, as the baseline, the seconds per image of the float64
restatement (tests/matte_eval_ref.py) on one CPU thread for the first CPU_IMAGES (2) images of the batch, whose sums are
compared with the device's.

Without arguments every case runs in a fresh child process under its own time limit, once per labelling schedule in
LEVELS (GGC_MATTE_EVAL_LEVELS; default "1 10"), and nothing is started after a failure.  `--case K` runs one case in
this process: the form to put under `rocprofv3 --kernel-trace --stats` in a run of its own for the per-kernel medians."""
import os
import subprocess
import sys
import time
from pathlib import Path

root = Path(__file__).resolve().parent.parent
CASES = ((256, 300, 400), (16, 600, 800))
REPS = int(os.environ.get("REPS", "5"))
CPU_IMAGES = int(os.environ.get("CPU_IMAGES", "2"))
STEP_TIMEOUT = int(os.environ.get("STEP_TIMEOUT", "240"))


def run_case(k: int) -> None:
    for p in (root, root / "src", root / "tests"):
        sys.path.insert(0, str(p))
    import numpy as np
    import torch
    from gcn_grabcut._engine import get_engine
    from gcn_grabcut.pipeline import ClosedFormMatte
    from gcn_grabcut.synthetic import synthetic_image
    from matte_eval_ref import matte_errors_ref

    B, H, W = CASES[k]
    eng = get_engine("cuda")
    imgs = np.stack([synthetic_image(H, W, 7000 + i % 16) for i in range(B)])
    bgr = eng.to_device(imgs)
    box = eng.to_device(np.broadcast_to(np.uint8(2), (B, H, W)).copy())         # GC_PR_BGD outside the box
    box[:, H // 8:H - H // 8, W // 8:W - W // 8] = 3                            # GC_PR_FGD inside
    mask = eng.grabcut(bgr, box, 5, 0, None, 0)[0].clone()
    to_u8 = lambda a: torch.floor(a.double() * 255.0 + 0.5).to(torch.uint8)     # noqa: E731
    pred = to_u8(eng.alpha_matte(bgr, mask))
    gt = to_u8(eng.closed_form_matte(bgr, mask, *ClosedFormMatte().args())[0])
    levels = os.environ.get("GGC_MATTE_EVAL_LEVELS", "default")
    for want_grad in (True, False):
        sums, grad, _ = eng.matte_errors(pred, gt, want_grad=want_grad)         # warm-up (scratch)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            sums, grad, _ = eng.matte_errors(pred, gt, want_grad=want_grad)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / REPS
        print(f"matte_errors B={B} {H}x{W} levels/pass {levels} grad={int(want_grad)}: {ms:.3f} ms per call, "
              f"{ms / B * 1e3:.1f} us per image", flush=True)
    sums, grad, _ = eng.matte_errors(pred, gt)
    sums, grad = sums.cpu().numpy(), grad.cpu().numpy()
    frac = ((pred > 0) & (pred < 255)).float().mean().item()
    print(f"  fractional pixels of pred {frac:.4f}; mean SAD {sums[:, 1].mean() / 255e3:.4f} GRAD {grad.mean() / 1e3:.4f} "
          f"CONN {sums[:, 3].mean() / 2550e3:.4f}", flush=True)
    # the model: per pixel and level, init reads a, g (2) and writes parent, area (8); merge reads parent and the row
    # above (8); area reads and writes parent (8) and touches area at the run starts; best reads parent (4); lev reads
    # parent and lev (5).  Per pixel once: sums reads a, g, lev (3); the stencil reads a, g (2) plus the halo's share.
    print(f"  bytes model (not counted): labelling 35 B x 10 levels + sums 3 B + stencil 2 B x {(24 * 24) / 256.0:.2f} "
          f"= {(350 + 3 + 2 * 2.25) * B * H * W / 1e9:.2f} GB per call", flush=True)
    p, g = pred[:CPU_IMAGES].cpu().numpy(), gt[:CPU_IMAGES].cpu().numpy()
    t0 = time.perf_counter()
    ref = [matte_errors_ref(p[i], g[i]) for i in range(len(p))]
    sec = (time.perf_counter() - t0) / max(1, len(p))
    for i, e in enumerate(ref):
        assert sums[i].tolist() == [e["n"], e["sad"], e["sse"], e["conn"]], (i, sums[i], e)
        assert abs(grad[i] - e["grad"]) <= 1e-9 * (1.0 + e["grad"]), (i, grad[i], e["grad"])
    print(f"  restatement on one CPU thread: {sec:.3f} s per image ({len(p)} images, sums equal to the device's)", flush=True)


def main() -> int:
    if len(sys.argv) == 3 and sys.argv[1] == "--case":
        run_case(int(sys.argv[2]))
        return 0
    for levels in os.environ.get("LEVELS", "1 10").split():
        for k in range(len(CASES)):
            env = dict(os.environ, GGC_MATTE_EVAL_LEVELS=levels)
            try:
                r = subprocess.run([sys.executable, __file__, "--case", str(k)], env=env, timeout=STEP_TIMEOUT)
            except subprocess.TimeoutExpired:
                print(f"case {k} (levels/pass {levels}) ran past {STEP_TIMEOUT} s: stopping", flush=True)
                return 124
            if r.returncode != 0:
                print(f"case {k} (levels/pass {levels}) ended with status {r.returncode}: stopping", flush=True)
                return r.returncode if r.returncode > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
