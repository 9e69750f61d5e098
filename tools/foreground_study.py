"""The float64 CPU study behind the foreground estimation's defaults: for each (eps_r, omega, tol) and
each alpha source (the true alpha, the closed-form matte and the guided matte at their defaults, as float32) the
iterations the preconditioned CG needs, and the premultiplied colour error of the clean cut-out over that of the
cut-out that keeps the image's bytes, on the soft disk (seeds 0, 1) and the strand scene.

    python3 tools/foreground_study.py [--max-iter 5000]

No device is used: the numbers come from tests/foreground_ref.py."""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

from foreground_ref import ALPHA_SOURCES, alpha_input, pcg, quality_ratio, scene_colours, snap  # noqa: E402
from matte_ref import edge_band  # noqa: E402

EVAL_BAND = 8          # the region scored: within 8 px of the mask's edge, as tools/closed_form_study.py
SCENES = (("disk", 0), ("disk", 1), ("strands", 0))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-iter", type=int, default=5000)
    ap.add_argument("--settings", type=float, nargs=3, action="append", metavar=("EPS_R", "OMEGA", "TOL"),
                    help="repeatable; default: the recorded table")
    a = ap.parse_args()
    settings = a.settings or [(5e-3, 1.0, 1e-6), (5e-3, 1.0, 1e-3), (1e-3, 1.0, 1e-6), (1e-5, 1.0, 1e-6),
                              (1e-2, 1.0, 1e-6), (5e-3, 0.1, 1e-6), (1e-2, 0.0, 1e-6)]
    names = [f"{k}{s}" for k, s in SCENES]
    print("| alpha | eps_r | omega | tol | " + " | ".join(f"{n} iters / ratio / colour err" for n in names) + " |")
    print("|---|---|---|---|" + "---|" * len(names))
    for source in ALPHA_SOURCES:
        for eps_r, omega, tol in settings:
            cells = []
            for kind, seed in SCENES:
                img, a_true, mask, fg, _ = scene_colours(kind, seed)
                alpha = alpha_input(kind, seed, source)
                F, _, it, rel = pcg(img, snap(alpha), eps_r, omega, a.max_iter, tol)
                ratio = quality_ratio(alpha, F, img, a_true, fg, edge_band(mask, EVAL_BAND))
                s = snap(alpha)
                sel = (a_true > 0.1) & (a_true < 1.0) & (s > 0) & (s < 1)
                before = np.abs(img - fg)[sel].mean()
                after = np.abs(255.0 * np.clip(F, 0.0, 1.0) - fg)[sel].mean()
                cells.append(f"{it}{'' if rel <= tol else '*'} / {ratio:.3f} / {before:.0f} -> {after:.1f}")
            print(f"| {source} | {eps_r:g} | {omega:g} | {tol:g} | " + " | ".join(cells) + " |", flush=True)
    print("\nratio = error(alpha', clamp F) / error(alpha, I), error(a, C) = sum |a C - alpha* F* / 255| over the region;"
          "\ncolour err = mean |colour - F*| in levels on 0.1 < alpha* < 1 within U, image -> estimate; * = max_iter reached")


if __name__ == "__main__":
    main()
