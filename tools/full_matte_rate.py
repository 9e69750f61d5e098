"""experiment helper: time and iterations of the warm full-size closed-form solve (ggc_trimap_matte_warm from the lifted
working-size alpha) next to the cold one (ggc_trimap_matte from 0.5) on the same lifted trimap.

    python3 tools/full_matte_rate.py --write DIR [--case NAME]     no device: scenes, working-size solve and lift by the
                                                                   restatement (tests/full_matte_ref.py) -> DIR/NAME.npz
    python3 tools/full_matte_rate.py --run DIR [--baseline]        device: ms per call and iterations per image

Cases: b16 = batch 16 of 1600x1200 lifted from 400x300 (4 strand scenes, each in its 4 flips); b4 = batch 4 of 4000x3000
lifted from 400x300.  --baseline runs the cold solve only, through nothing but Engine.trimap_matte(alpha0=None), so that
the same file run from a checkout of the parent commit reads the same trimaps and gives the baseline.  Time per call
from events over REPS calls after a warm-up."""
import argparse
import os
import sys
from pathlib import Path

import numpy as np

root = Path(__file__).resolve().parent.parent
CASES = {"b16": (16, 1200, 1600, 4), "b4": (4, 3000, 4000, 10)}          # batch, H1, W1, box-down factor
R, EPS, MAX_ITER, TOL = 1, 1e-5, 2000, 1e-4


def write(out_dir: Path, names):
    sys.path.insert(0, str(root / "tests"))
    import full_matte_ref as fm
    import trimap_matte_ref as tm
    from closed_form_ref import pcg as band_pcg
    out_dir.mkdir(parents=True, exist_ok=True)
    r, eps, band, max_iter, tol = fm.CF
    for name in names:
        b, h1, w1, k = CASES[name]
        fulls, tris, starts = [], [], []
        for seed in range(4):
            full, _, work, mask = fm.full_scene(h1, w1, k, seed)
            wa, it, _ = band_pcg(work, mask, r, eps, band, max_iter, tol)
            t_full, a0 = fm.lift(tm.trimap_from_mask(mask, band), wa, (h1, w1), 0)
            print(f"{name} seed {seed}: working solve {it} iterations, lifted unknown {np.mean(t_full == 128):.4f}", flush=True)
            flips = (slice(None), slice(None, None, -1))
            for fy, fx in [(y, x) for y in flips for x in flips][: b // 4]:
                fulls.append(full[fy, fx]); tris.append(t_full[fy, fx]); starts.append(a0[fy, fx])
        np.savez(out_dir / f"{name}.npz", full=np.stack(fulls), trimap=np.stack(tris), alpha0=np.stack(starts))


def run(in_dir: Path, names, baseline: bool):
    sys.path.insert(0, str(root))
    sys.path.insert(0, str(root / "src"))
    import torch
    from gcn_grabcut._engine import get_engine
    reps = int(os.environ.get("REPS", "2"))
    eng = get_engine("cuda")

    def timed(fn):
        out = fn()                                                               # warm-up (scratch)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps, out

    for name in names:
        z = np.load(in_dir / f"{name}.npz")
        bgr, tri, a0 = eng.to_device(z["full"]), eng.to_device(z["trimap"]), eng.to_device(z["alpha0"])
        alpha = eng.empty(*tri.shape)
        runs = [("cold (0.5)", dict(alpha0=None))]
        if not baseline:
            runs.append(("warm (lifted)", dict(alpha0=a0, warm=True)))
        for what, kw in runs:
            ms, (_, iters, rel) = timed(lambda: eng.trimap_matte(bgr, tri, R, EPS, MAX_ITER, TOL, out=(alpha, None), **kw))
            it = iters.cpu().numpy()
            print(f"{name} B={tri.shape[0]} {tri.shape[1]}x{tri.shape[2]} {what}: {ms:.1f} ms per call; iterations per image "
                  f"min {it.min()} median {int(np.median(it))} max {it.max()}; rel_residual max {rel.max().item():.2e}",
                  flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--write", metavar="DIR")
    mode.add_argument("--run", metavar="DIR")
    ap.add_argument("--case", choices=sorted(CASES), action="append")
    ap.add_argument("--baseline", action="store_true")
    args = ap.parse_args()
    cases = args.case or sorted(CASES, reverse=True)
    if args.write:
        write(Path(args.write), cases)
    else:
        run(Path(args.run), cases, args.baseline)
