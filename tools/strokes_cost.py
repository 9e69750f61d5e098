"""Cost of the brush strokes at the benchmark's shape: a batch of 256 images at 400x300 with 8 strokes of 6
vertices per image (4 foreground, 4 background; 40 segments), brush radius 5.  Timed: ggc_apply_strokes, ggc_stroke_pixels
(the count call, the read of the total and the fill call), ggc_apply_hints with 32 clicks per image for scale, and
ggc_geodesic_hints on the strokes' centre-line pixels as its click list (k_geo_seed scans the later clicks of an image per
click, so its cost grows with the square of the stroke pixels per image).

    rocprofv3 --kernel-trace --stats -d <dir> -o strokes -- python3 tools/strokes_cost.py

The kernel times come from the profiler's summary; the lines printed here are host wall times per call (they include the
synchronising reads of stroke_ptr and the segments)."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "src")]

from gcn_grabcut._engine import get_engine                          # noqa: E402
from gcn_grabcut.graph_builder import pack_hints, pack_strokes      # noqa: E402


def scribble(rng, h, w, n_vertices, step):
    """A polyline that starts inside the image and moves by at most `step` pixels per vertex (it may leave the frame)."""
    v = [(int(rng.integers(0, h)), int(rng.integers(0, w)))]
    for _ in range(n_vertices - 1):
        v.append((v[-1][0] + int(rng.integers(-step, step + 1)), v[-1][1] + int(rng.integers(-step, step + 1))))
    return v


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
    ap.add_argument("--strokes", type=int, default=8)
    ap.add_argument("--vertices", type=int, default=6)
    ap.add_argument("--step", type=int, default=60, help="largest move per vertex along each axis, in pixels")
    ap.add_argument("--radius", type=int, default=5)
    ap.add_argument("--clicks", type=int, default=32)
    ap.add_argument("--geodesic-batch", type=int, default=64, help="images of the geodesic leg (0 = skip it)")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    b, h, w = args.batch, args.height, args.width
    eng = get_engine("cuda")
    rng = np.random.default_rng(0)
    mask = eng.to_device(rng.integers(0, 4, (b, h, w)).astype(np.uint8))
    half = args.strokes // 2
    per_image = []
    for _ in range(b):
        s = [scribble(rng, h, w, args.vertices, args.step) for _ in range(args.strokes)]
        per_image.append((s[:half], s[half:]))
    segs, seg_ptr = pack_strokes(per_image)
    strokes, stroke_ptr = eng.upload_strokes(segs, seg_ptr)
    pix, pix_ptr = eng.stroke_pixels((b, h, w), strokes, stroke_ptr)
    print(f"{b} images {h}x{w}: {len(segs) / b:.0f} segments and {pix.size(0) / b:.0f} centre-line pixels per image, "
          f"brush radius {args.radius}", flush=True)
    timed("ggc_apply_strokes", lambda: eng.apply_strokes(mask, strokes, stroke_ptr, args.radius), args.reps)
    timed("ggc_stroke_pixels (count + fill)", lambda: eng.stroke_pixels((b, h, w), strokes, stroke_ptr), args.reps)
    clicks = [([(int(rng.integers(0, h)), int(rng.integers(0, w))) for _ in range(args.clicks // 2)],
               [(int(rng.integers(0, h)), int(rng.integers(0, w))) for _ in range(args.clicks - args.clicks // 2)])
              for _ in range(b)]
    hints, hint_ptr = eng.upload_hints(*pack_hints(clicks))
    timed(f"ggc_apply_hints ({args.clicks} clicks, radius {args.radius})",
          lambda: eng.apply_hints(mask, hints, hint_ptr, args.radius), args.reps)
    gb = min(args.geodesic_batch, b)
    if gb > 0:
        from gcn_grabcut.synthetic import synthetic_batch
        bgr = eng.to_device(synthetic_batch(gb, h, w, config_id=3))
        n = int(pix_ptr[gb].item())
        g_rows, g_ptr = pix[:n].contiguous(), pix_ptr[:gb + 1].contiguous()
        print(f"geodesic leg: {gb} images, {n / gb:.0f} sources per image", flush=True)
        timed("ggc_geodesic_hints (centre lines as sources, radius 40, gamma 2)",
              lambda: eng.geodesic_hints(bgr, g_rows, g_ptr, 40, 2, mask=mask[:gb]), max(args.reps // 4, 2))


if __name__ == "__main__":
    main()
