"""The float64 CPU study behind the closed-form matte's defaults: for each (radius, eps, band) the
iterations Jacobi-PCG needs to reach tol, and the SAD to the true alpha over the scene's edge region, on the soft disk
(seeds 0, 1) and the strand scene, next to the guided matte's (alpha_matte at its defaults) and the hard mask's.

    python3 tools/closed_form_study.py [--tol 1e-4] [--max-iter 2000]

No device is used: the numbers come from tests/closed_form_ref.py."""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

from closed_form_ref import band_sad, pcg, strand_scene  # noqa: E402
from matte_ref import alpha_matte_ref, edge_band, soft_disk_scene  # noqa: E402

EVAL_BAND = 8          # the region scored: within 8 px of the mask's edge (the guided matte's 2r at its defaults)


def scenes():
    for seed in (0, 1):
        yield f"disk{seed}", soft_disk_scene(120, 160, 40.0, 3.0, seed)
    yield "strands0", strand_scene(120, 160, seed=0)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--max-iter", type=int, default=2000)
    ap.add_argument("--radii", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--eps", type=float, nargs="+", default=[1e-7, 1e-5, 1e-3])
    ap.add_argument("--bands", type=int, nargs="+", default=[4, 8])
    a = ap.parse_args()
    cases = list(scenes())
    print("| scene | hard mask SAD | guided SAD (r 4, eps 1e-4) |")
    print("|---|---|---|")
    base = {}
    for name, (img, at, m) in cases:
        region = edge_band(m, EVAL_BAND)
        base[name] = band_sad(alpha_matte_ref(img, m, 4, 1e-4), at, region)
        print(f"| {name} | {band_sad(m, at, region):.1f} | {base[name]:.1f} |")
    print()
    print("| r | eps | band | " + " | ".join(f"{n} iters / SAD / ratio" for n, _ in cases) + " |")
    print("|---|---|---|" + "---|" * len(cases))
    for r in a.radii:
        for eps in a.eps:
            for band in a.bands:
                cells = []
                for name, (img, at, m) in cases:
                    x, it, rel = pcg(img, m, r, eps, band, a.max_iter, a.tol)
                    sad = band_sad(np.clip(x, 0.0, 1.0), at, edge_band(m, EVAL_BAND))
                    cells.append(f"{it}{'' if rel <= a.tol else '*'} / {sad:.1f} / {sad / base[name]:.2f}")
                print(f"| {r} | {eps:g} | {band} | " + " | ".join(cells) + " |")
    print("\n* = max_iter reached before tol")


if __name__ == "__main__":
    main()
