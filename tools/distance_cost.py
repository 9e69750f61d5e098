"""Cost of the exact distance transform and the mask modifiers on the masks of the benchmark's scenes.

    python3 tools/distance_cost.py                     HIP-event timings against a streaming floor, and the split by pass
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 tools/distance_cost.py --calls 5
                                                       the per-kernel split, in a run of its own (then --stats-csv <file>)
    python3 tools/distance_cost.py --stats-csv <dir>/.../*kernel_stats.csv        prints the distance kernels of that summary

The batch is 256 masks of 400x300: the ground-truth masks of the bench scenes (synthetic_image(300, 400, 30000 + i,
return_mask=True)).  Timed by HIP events around the call on the stream, 3 warm-up + 20 calls, median (min-max).

The yardstick is a streaming floor: the bytes a step MUST move (the mask read once, 1 B per pixel; the 16-bit g written by
the column pass and read by the row pass, 2 + 2 B; the result written, 4 B as int32 or 1 B as u8) divided by HBM_RATE, the
float4-copy rate of HBM measured on this part.  The batch (31 MB of mask, 61 MB of g, 123 MB of int32) fits the 256 MiB
last-level cache, so a call can beat the floor; it is a yardstick for "how many passes over the data does this cost", not a
bound.  The column pass as written moves more than it must: it reads the mask in both sweeps and writes and re-reads g
between them (1 + 1 + 2 + 2 + 2 B per pixel instead of 1 + 2); that figure is printed beside the floor."""
import argparse
import csv
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "src")]

HBM_RATE = 6.29e12          # bytes per second: measured float4 copy on MI355X (8.0 TB/s on the data sheet)
SCOPES = ("distance_cols", "distance_rows")
GROW, OPEN, TRIMAP = 0, 3, 5


def median_ms(fn, warm=3, reps=20):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times)), float(max(times))


def stats(path):
    rows = [r for r in csv.DictReader(open(path)) if "k_dt_" in r["Name"]]
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print(f"kernel | calls | total ms | average us | share   ({path})")
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        name = re.search(r"k_dt_\w+(<[^>]*>)?", r["Name"]).group(0)
        print(f"{name} | {r['Calls']} | {float(r['TotalDurationNs']) / 1e6:.3f} | {float(r['AverageNs']) / 1e3:.1f} | "
              f"{100 * float(r['TotalDurationNs']) / total:.1f} %")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=0, help="for a profiler run: this many plain calls per row, no timing")
    ap.add_argument("--stats-csv", default=None, help="print the distance kernels of a rocprofv3 kernel_stats.csv and exit")
    args = ap.parse_args()
    if args.stats_csv:
        return stats(args.stats_csv)
    import torch
    from gcn_grabcut._engine import get_engine
    from gcn_grabcut.synthetic import synthetic_image
    eng = get_engine("cuda")
    b, h, w = args.batch, 300, 400
    masks = eng.to_device(np.stack([synthetic_image(h, w, 30000 + i, return_mask=True)[1] for i in range(b)]).astype(np.uint8))
    worst = torch.ones_like(masks)
    worst[:, 0, 0] = 0                                                  # one background pixel in a full image
    n = b * h * w
    d2 = torch.empty((b, h, w), dtype=torch.int32, device="cuda")
    u8 = torch.empty_like(masks)
    fg = float(masks.float().mean().item())
    print(f"## {b} x {h}x{w} masks of the bench scenes, {100 * fg:.1f} % foreground; HBM_RATE {HBM_RATE / 1e12:.2f} TB/s", flush=True)

    def dist(m, cap):
        return lambda: eng.mask_distance(m, False, cap, out=d2)

    def mod(op, a, c=0):
        return lambda: eng.modify_mask(masks, op, a, c, out=u8)

    # name, call, steps, result bytes per pixel of the last step (a first step of two writes a u8 plane)
    rows = [("ggc_mask_distance, unbounded", dist(masks, 0), 1, 4),
            ("ggc_mask_distance, max_dist2 = 9", dist(masks, 9), 1, 4),
            ("ggc_mask_distance, max_dist2 = 64", dist(masks, 64), 1, 4),
            ("ggc_modify_mask GROW, r2 = 9", mod(GROW, 9), 1, 1),
            ("ggc_modify_mask OPEN, r2 = 9", mod(OPEN, 9), 2, 1),
            ("ggc_modify_mask TRIMAP, (9, 64)", mod(TRIMAP, 9, 64), 1, 1),
            ("ggc_mask_distance, unbounded, WORST CASE: one background pixel in a full image", dist(worst, 0), 1, 4)]
    if args.calls:                                                      # under the profiler: a few plain calls and nothing else
        for _, fn, _, _ in rows:
            for _ in range(args.calls):
                fn()
        torch.cuda.synchronize()
        return
    print("call | median ms | min | max | floor ms | median / floor | as written ms | cols ms | rows ms"
          "   (HIP events, 3 warm-up + 20 calls; the two passes by ggc_profile_query on one more call)")
    for name, fn, steps, out_bytes in rows:
        must = n * ((1 + 2 + 2) * steps + (steps - 1) * 1 + out_bytes)
        written = n * ((1 + 1 + 2 + 2 + 2 + 2) * steps + (steps - 1) * 1 + out_bytes)
        med, lo, hi = median_ms(fn)
        eng.ctx.profile_enable(1)
        fn()
        cols, rows_ms = (eng.ctx.profile_query(s)[1] for s in SCOPES)
        eng.ctx.profile_enable(0)
        floor = 1e3 * must / HBM_RATE
        print(f"{name} | {med:.3f} | {lo:.3f} | {hi:.3f} | {floor:.3f} | {med / floor:.1f} | {1e3 * written / HBM_RATE:.3f} | "
              f"{cols:.3f} | {rows_ms:.3f}", flush=True)


if __name__ == "__main__":
    main()
