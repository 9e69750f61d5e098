"""The float64 CPU study behind the trimap matte's tests and DESIGN.md §5.16: on the strand scenes (seeds 0, 1, 2) and
the soft disk, with the trimap's unknown region U the Chebyshev dilation by k of {0 < alpha* < 1}, the iterations
Jacobi-PCG needs from 0.5, the SAD over U of the trimap solve, of the mask-band matte at its defaults and of the hard mask,
and (--tau) the distance between the solve at the default tol and the solve at 1e-12 over the cases the GPU test runs.

    python3 tools/trimap_matte_study.py [--tau] [--large]

No device is used: the numbers come from tests/trimap_matte_ref.py and tests/closed_form_ref.py."""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import closed_form_ref as cf  # noqa: E402
import trimap_matte_ref as tm  # noqa: E402
from matte_ref import soft_disk_scene  # noqa: E402

R, EPS, BAND, MAX_ITER, TOL = 1, 1e-5, 1, 500, 1e-4          # pipeline.CF_*


def scenes():
    for seed in (0, 1, 2):
        yield f"strands{seed}", cf.strand_scene(120, 160, seed=seed)
    yield "disk0", soft_disk_scene(120, 160, 40.0, 3.0, 0)


def row(name, img, at, mask, k, max_iter):
    t = tm.trimap_from_alpha(at, k)
    U = tm.regions(t)[2]
    x, it, rel = tm.pcg(img, t, R, EPS, max_iter, TOL)
    band, _, _ = cf.pcg(img, mask, R, EPS, BAND, MAX_ITER, TOL)
    s_t, s_b = tm.region_sad(np.clip(x, 0, 1), at, U), tm.region_sad(np.clip(band, 0, 1), at, U)
    s_m = tm.region_sad(mask, at, U)
    print(f"| {name} | {k} | {100.0 * U.mean():.0f} % | {it}{'' if rel <= TOL else '*'} | {s_t:.1f} | {s_b:.1f} | {s_m:.1f} | "
          f"{s_t / s_b:.3f} | {s_t / s_m:.3f} |", flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tau", action="store_true", help="also measure |pcg(tol 1e-4) - pcg(tol 1e-12)| over the GPU test's cases")
    ap.add_argument("--large", action="store_true", help="also strands0 at 240x320")
    ap.add_argument("--max-iter", type=int, default=2000)
    a = ap.parse_args()
    print("| scene | k | unknown share | CG iterations (start 0.5) | SAD, trimap solve | SAD, mask-band matte | SAD, hard mask | "
          "trimap / band | trimap / mask |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, (img, at, mask) in scenes():
        for k in (1, 2, 3, 10):
            row(name, img, at, mask, k, a.max_iter)
    if a.large:
        img, at, mask = cf.strand_scene(240, 320, radius=80.0, seed=0)
        for k in (2, 10):
            row("strands0 240x320", img, at, mask, k, a.max_iter)
    print("\n* = max_iter reached before tol")
    if a.tau:
        worst = 0.0
        print("\n| scene | k | r | start | iterations at 1e-4 | max abs difference to 1e-12 |")
        print("|---|---|---|---|---|---|")
        for name, (img, at, mask) in scenes():
            for k in (1, 2, 3, 10):
                t = tm.trimap_from_alpha(at, k)
                for r in (1, 2):
                    for a0 in (None, mask.astype(np.float32)):
                        x, it, _ = tm.pcg(img, t, r, EPS, a.max_iter, TOL, a0)
                        y, _, rel = tm.pcg(img, t, r, EPS, 50000, 1e-12, a0)
                        assert rel <= 1e-12
                        e = float(np.abs(x - y).max())
                        worst = max(worst, e)
                        print(f"| {name} | {k} | {r} | {'0.5' if a0 is None else 'mask'} | {it} | {e:.4f} |", flush=True)
        print(f"\nmax over the cases: {worst:.4f}; tau = twice that = {2 * worst:.4f}")


if __name__ == "__main__":
    main()
