"""Cost of mask outlines on the masks of the benchmark's workload.

    python3 tools/outlines_cost.py                     HIP-event timings and the split by ggc_profile_query
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 tools/outlines_cost.py --calls 5
                                                       the per-kernel split, in a run of its own (then --stats-csv <file>)
    python3 tools/outlines_cost.py --stats-csv <dir>/.../*kernel_stats.csv        prints the outline kernels of that summary

(a) the batch of 256 masks of 400x300 that segment_batch_device produces for the bench scenes (config 3, seeds 30000..), and
(b) one 3000x4000 mask: image 0's mask of that batch, every pixel repeated 10 x 10.  Timed by HIP events around the call on the
stream, 3 warm-up + 20 calls, median (min-max): Engine.mask_outlines (a counting and a filling call of the exact size), the
count-only call, ggc_clean_mask on the same masks (the sibling post stage), and on (a) the batch step that made the masks.
ggc_mask_outlines reads its totals back, so its times include those synchronisations."""
import argparse
import csv
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "src")]

SCOPES = ("outline_mark", "outline_scan", "outline_fill", "outline_jump", "outline_loops", "outline_label", "outline_emit")


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
    rows = [r for r in csv.DictReader(open(path)) if "k_ol_" in r["Name"]]
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print(f"kernel | calls | total ms | average us | share   ({path})")
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        name = re.search(r"k_ol_\w+(<[^>]*>)?", r["Name"]).group(0)
        print(f"{name} | {r['Calls']} | {float(r['TotalDurationNs']) / 1e6:.3f} | {float(r['AverageNs']) / 1e3:.1f} | "
              f"{100 * float(r['TotalDurationNs']) / total:.1f} %")


def measure(eng, what, masks, connectivity, calls, step=None):
    import torch
    b, h, w = masks.shape
    verts, loop_ptr, info, image_ptr, image_vert_ptr = eng.mask_outlines(masks, connectivity)
    q, v = int(info.shape[0]), int(verts.shape[0])
    cracks = int(info[:, 2].sum().item())
    per_image = torch.zeros(b, dtype=torch.int64, device=masks.device)
    per_image.index_add_(0, torch.bucketize(torch.arange(q, device=masks.device), image_ptr[1:].long(), right=True),
                         info[:, 2].long())
    most = int(per_image.max().item())
    print(f"## {what}: {b} x {h}x{w}, connectivity {connectivity}: {cracks} cracks, {q} loops, {v} vertices; longest loop "
          f"{int(info[:, 2].max().item())} cracks; most cracks in one image {most} -> {max(1, int(np.ceil(np.log2(most))))} doubling rounds",
          flush=True)
    if calls:                                                           # under the profiler: a few plain calls and nothing else
        for _ in range(calls):
            eng.mask_outlines(masks, connectivity)
        torch.cuda.synchronize()
        return
    ip, ivp = torch.zeros_like(image_ptr), torch.zeros_like(image_vert_ptr)
    out = torch.empty_like(masks)
    rows = [("Engine.mask_outlines (count, then fill)", lambda: eng.mask_outlines(masks, connectivity)),
            ("ggc_mask_outlines, filling call with the capacities known", lambda: eng.ctx.call(
                "ggc_mask_outlines", eng._stream(), b, h, w, masks.data_ptr(), connectivity, ip.data_ptr(), ivp.data_ptr(),
                loop_ptr.data_ptr(), info.data_ptr(), verts.data_ptr(), q, v)),
            ("ggc_mask_outlines, count only", lambda: eng.ctx.call(
                "ggc_mask_outlines", eng._stream(), b, h, w, masks.data_ptr(), connectivity, ip.data_ptr(), ivp.data_ptr(),
                None, None, None, 0, 0)),
            ("ggc_clean_mask (min_area_ratio 0.002)", lambda: eng.clean_mask(masks, 0.002, False, out=out))]
    if step is not None:
        rows.append(("segment_batch_device, the batch step", step))
    print("call | median ms | min | max   (HIP events, 3 warm-up + 20 calls)")
    med = {}
    for name, fn in rows:
        med[name], lo, hi = median_ms(fn)
        print(f"{name} | {med[name]:.3f} | {lo:.3f} | {hi:.3f}", flush=True)
    if step is not None:
        share = 100 * med[rows[1][0]] / med[rows[-1][0]]
        print(f"the filling call is {share:.2f} % of the batch step (the standing target for an optional stage: under 1 %)")
    eng.ctx.profile_enable(1)
    eng.ctx.call("ggc_mask_outlines", eng._stream(), b, h, w, masks.data_ptr(), connectivity, ip.data_ptr(), ivp.data_ptr(),
                 loop_ptr.data_ptr(), info.data_ptr(), verts.data_ptr(), q, v)
    print("part of one filling call | launches | total ms   (HIP events around each scope)")
    for name in SCOPES:
        launches, ms = eng.ctx.profile_query(name)
        print(f"{name} | {launches} | {ms:.3f}", flush=True)
    eng.ctx.profile_enable(0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--connectivity", type=int, default=8, choices=[4, 8])
    ap.add_argument("--calls", type=int, default=0, help="for a profiler run: this many plain calls per case, no timing")
    ap.add_argument("--stats-csv", default=None, help="print the outline kernels of a rocprofv3 kernel_stats.csv and exit")
    args = ap.parse_args()
    if args.stats_csv:
        return stats(args.stats_csv)
    import torch
    from gcn_grabcut.graph_builder import SuperpixelGraphConfig
    from gcn_grabcut.model import ResGCNNet
    from gcn_grabcut.pipeline import GCNGrabCutPipeline
    from gcn_grabcut.synthetic import synthetic_batch
    torch.manual_seed(0)                                                # bench.py's model, scenes and pipeline
    model = ResGCNNet(hidden_channels=128, n_layers=6).to("cuda").eval()
    pipe = GCNGrabCutPipeline(model, sp_config=SuperpixelGraphConfig(n_segments=600), device="cuda:0", grabcut_lanes=4)
    bgr = torch.from_numpy(synthetic_batch(args.batch, 300, 400, config_id=3, first_index=0)).to("cuda")
    masks = pipe.segment_batch_device(bgr, compose=True)["binary_mask"].contiguous()
    eng = pipe._eng
    measure(eng, "(a) the bench batch", masks, args.connectivity, args.calls,
            step=lambda: pipe.segment_batch_device(bgr, compose=True))
    big = masks[:1].repeat_interleave(10, dim=1).repeat_interleave(10, dim=2).contiguous()
    measure(eng, "(b) image 0's mask, 10 x 10", big, args.connectivity, args.calls)


if __name__ == "__main__":
    main()
