"""experiment helper: the float64 study behind the full-resolution closed-form matte.

    python3 tools/full_matte_study.py [--quality] [--grow] [--tau]        (no flag: all three)

No device is used: the numbers come from tests/full_matte_ref.py (the lift and the warm stop rule restated in numpy)
over closed_form_ref.py, trimap_matte_ref.py and upsample_ref.py.

  --quality  strand scenes at 480x640 from the 120x160 working size (4x4 box-down), working-size closed-form matte at
             its defaults: whole-image SAD against the true alpha of the upsampled hard mask, of upsample_mask's alpha
             (r 8, eps 1e-4), of the working alpha interpolated bilinearly (the lifted start) and of the full-size solve
             on the lifted trimap; iterations of that solve warm (stop against the 0.5 start's residual) and cold (from
             0.5), and max |warm - cold|
  --grow     seed 0: SAD, cold and warm iterations with the lifted unknown region grown by 0, 4, 8 and 16 pixels
  --tau      max |solve at tol 1e-4 - solve at tol 1e-12| of the warm restatement over full_matte_ref.WARM_CASES, the
             cases the GPU test runs; the test's bound is twice that"""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
import full_matte_ref as fm  # noqa: E402
import trimap_matte_ref as tm  # noqa: E402
from upsample_ref import upsample_ref  # noqa: E402


def nearest(a, h1, w1):
    h, w = a.shape
    ys = np.minimum(((np.arange(h1) + 0.5) * h / h1).astype(np.int64), h - 1)
    xs = np.minimum(((np.arange(w1) + 0.5) * w / w1).astype(np.int64), w - 1)
    return a[ys][:, xs]


def quality():
    print("seed | hard mask up | upsample_mask alpha | working alpha bilinear | full-size solve | ratio | warm it | cold it | max|warm-cold|")
    for seed in (0, 1):
        full, at, work, mask = fm.full_scene(480, 640, 4, seed)
        warm = fm.chain(full, work, mask)
        cold = fm.chain(full, work, mask, warm=False)
        s_mask = fm.sad(nearest(mask, 480, 640), at)
        s_up = fm.sad(upsample_ref(work, mask, full, 8, 1e-4), at)
        s_bil = fm.sad(warm["alpha0_full"], at)
        s_full = fm.sad(warm["alpha"], at)
        print(f"{seed} | {s_mask:.0f} | {s_up:.0f} | {s_bil:.0f} | {s_full:.0f} | {s_full / s_mask:.4f} | {warm['iters']} | "
              f"{cold['iters']} | {np.abs(warm['alpha'] - cold['alpha']).max():.4f}", flush=True)


def grow():
    print("grow | SAD (cold) | cold it | SAD (warm) | warm it")
    full, at, work, mask = fm.full_scene(480, 640, 4, 0)
    for g in (0, 4, 8, 16):
        warm = fm.chain(full, work, mask, grow=g)
        cold = fm.chain(full, work, mask, grow=g, warm=False)
        print(f"{g} | {fm.sad(cold['alpha'], at):.0f} | {cold['iters']} | {fm.sad(warm['alpha'], at):.0f} | {warm['iters']}",
              flush=True)


def tau():
    worst = 0.0
    r, eps = fm.CF[0], fm.CF[1]
    for case in fm.WARM_CASES:
        full, t_full, a0 = fm.warm_case(*case)
        a, it, _ = fm.pcg_warm(full, t_full, r, eps, fm.FULL_MAX_ITER, 1e-4, a0)
        b, it_b, rel_b = fm.pcg_warm(full, t_full, r, eps, 20000, 1e-12, a0)
        d = float(np.abs(a - b).max())
        worst = max(worst, d)
        print(f"{case}: unknown {int(tm.regions(t_full)[2].sum())}, {it} iterations at 1e-4, {it_b} at 1e-12 (rel {rel_b:.1e}), "
              f"max |difference| {d:.4f}", flush=True)
    print(f"TAU_MEASURED = {worst:.4f}; the GPU test holds the device within 2 x that")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--grow", action="store_true")
    ap.add_argument("--tau", action="store_true")
    args = ap.parse_args()
    every = not (args.quality or args.grow or args.tau)
    if args.tau or every:
        tau()
    if args.quality or every:
        quality()
    if args.grow or every:
        grow()
