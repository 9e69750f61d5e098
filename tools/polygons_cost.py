"""Cost of lassos and filled polygons at the benchmark's shape: a batch of 256 images at 400x300 with one
24-vertex lasso plus two 8-vertex fills per image (one foreground, one background; 40 edges).  Timed: ggc_apply_polygons,
and for scale ggc_apply_strokes with 40 segments per image and ggc_apply_hints with 32 clicks per image.

    rocprofv3 --kernel-trace --stats -d <dir> -o polygons -- python3 tools/polygons_cost.py

The kernel times come from the profiler's summary; the lines printed here are host wall times per call (they include the
synchronising reads of the four polygon arrays)."""
import argparse
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "src")]

from gcn_grabcut._engine import get_engine                                          # noqa: E402
from gcn_grabcut.graph_builder import pack_hints, pack_polygons, pack_strokes       # noqa: E402


def blob(rng, cy, cx, ry, rx, n_vertices):
    """A star-shaped outline of n vertices around (cy, cx): radii between 60 % and 100 % of (ry, rx); it may leave the frame."""
    out = []
    for i in range(n_vertices):
        a, s = 2 * math.pi * i / n_vertices, rng.uniform(0.6, 1.0)
        out.append((int(round(cy + s * ry * math.sin(a))), int(round(cx + s * rx * math.cos(a)))))
    return out


def timed(what, fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    print(f"{what}: {(time.perf_counter() - t0) * 1e3 / reps:.3f} ms per call (host wall)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--height", type=int, default=300)
    ap.add_argument("--width", type=int, default=400)
    ap.add_argument("--lasso-vertices", type=int, default=24)
    ap.add_argument("--fills", type=int, default=2)
    ap.add_argument("--fill-vertices", type=int, default=8)
    ap.add_argument("--clicks", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    b, h, w = args.batch, args.height, args.width
    eng = get_engine("cuda")
    rng = np.random.default_rng(0)
    mask = eng.to_device(rng.integers(0, 4, (b, h, w)).astype(np.uint8))
    per_image = []
    for _ in range(b):
        lasso = blob(rng, h / 2 + rng.integers(-20, 21), w / 2 + rng.integers(-20, 21), 0.55 * h, 0.55 * w, args.lasso_vertices)
        fills = [blob(rng, rng.integers(0, h), rng.integers(0, w), h / 8, w / 8, args.fill_vertices) for _ in range(args.fills)]
        per_image.append((fills[:(args.fills + 1) // 2], fills[(args.fills + 1) // 2:], [lasso]))
    packed = pack_polygons(per_image)
    polys = eng.upload_polygons(*packed)
    print(f"{b} images {h}x{w}: {len(packed[2]) / b:.0f} polygons and {len(packed[0]) / b:.0f} edges per image", flush=True)
    timed("ggc_apply_polygons", lambda: eng.apply_polygons(mask, *polys), args.reps)
    n_seg = len(packed[0]) // b
    strokes = [([[(int(rng.integers(0, h)), int(rng.integers(0, w))) for _ in range(n_seg + 1)]], []) for _ in range(b)]
    segs, seg_ptr = eng.upload_strokes(*pack_strokes(strokes))
    timed(f"ggc_apply_strokes ({n_seg} segments, radius 5)", lambda: eng.apply_strokes(mask, segs, seg_ptr, 5), args.reps)
    clicks = [([(int(rng.integers(0, h)), int(rng.integers(0, w))) for _ in range(args.clicks // 2)],
               [(int(rng.integers(0, h)), int(rng.integers(0, w))) for _ in range(args.clicks - args.clicks // 2)])
              for _ in range(b)]
    hints, hint_ptr = eng.upload_hints(*pack_hints(clicks))
    timed(f"ggc_apply_hints ({args.clicks} clicks, radius 5)", lambda: eng.apply_hints(mask, hints, hint_ptr, 5), args.reps)


if __name__ == "__main__":
    main()
