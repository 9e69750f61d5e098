"""Cost of the click simulation: ggc_next_click and one whole click round at the benchmark's shape, a batch of
256 images at 400x300.  The masks are the automatic pipeline's GrabCut result on synthetic images against their ground
truth, so the error regions are the ones a click evaluation starts from.

    rocprofv3 --kernel-trace --stats -d <dir> -o clicks -- python3 tools/click_cost.py

The kernel times come from the profiler's summary; the lines printed here are host wall times around synchronised calls
(a round includes ggc_apply_hints' read of hint_ptr and the read of the IoU vector)."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "src")]

from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig   # noqa: E402
from gcn_grabcut.model import ResGCNNet                             # noqa: E402
from gcn_grabcut.synthetic import synthetic_image                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--height", type=int, default=300)
    ap.add_argument("--width", type=int, default=400)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--radius", type=int, default=5)
    args = ap.parse_args()
    b, h, w = args.batch, args.height, args.width
    torch.manual_seed(0)
    pipe = GCNGrabCutPipeline(ResGCNNet(hidden_channels=128, n_layers=6).eval(),
                              sp_config=SuperpixelGraphConfig(n_segments=300), device="cuda")
    eng = pipe._eng
    pairs = [synthetic_image(h, w, i, return_mask=True) for i in range(b)]
    gt = eng.to_device(np.stack([m for _, m in pairs]).astype(np.uint8))
    out = pipe.segment_batch_device(eng.to_device(np.stack([im for im, _ in pairs])), compose=False, return_state=True)
    binary, mask, bgd, fgd, image = out["gc_binary"], out["gc_mask"], out["bgd"], out["fgd"], out["gc_image"]
    err = (binary != gt).float().mean().item()
    d2 = eng.next_click(binary, gt)[:, 3].float()
    print(f"start: {err:.1%} of the pixels wrong, largest error region d2 median {d2.median().item():.0f}, "
          f"max {d2.max().item():.0f}", flush=True)

    for _ in range(3):
        eng.next_click(binary, gt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        eng.next_click(binary, gt)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.reps
    print(f"next_click: {ms:.3f} ms per call (host wall, {b} images {h}x{w})", flush=True)

    ptr = torch.arange(b + 1, dtype=torch.int32, device=eng.device)
    for r in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        click, binary, mask, bgd, fgd, iou = pipe._click_round(binary, gt, mask, image, bgd, fgd, ptr, args.radius, 1)
        miou = iou.mean().item()
        ms = (time.perf_counter() - t0) * 1e3
        print(f"round {r + 1}: {ms:.2f} ms (host wall: next_click + apply_hints + 1 GC_EVAL iteration + IoU), "
              f"mIoU {miou:.4f}, {(click[:, 0] >= 0).sum().item()} clicks", flush=True)


if __name__ == "__main__":
    main()
