"""Cost of ggc_apply_hints at the benchmark's shape: a batch of 256 images at 400x300 with 32 clicks per image
(16 foreground, 16 background, radius 5) and a ~300-region label map, in both region modes.

    rocprofv3 --kernel-trace --stats -d <dir> -o hints -- python3 tools/hints_cost.py

The kernel times come from the profiler's summary; the line printed here is the host wall time of one call (it includes the
synchronising read of hint_ptr / node_ptr)."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "src")]

from gcn_grabcut._engine import get_engine          # noqa: E402
from gcn_grabcut.graph_builder import pack_hints    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--height", type=int, default=300)
    ap.add_argument("--width", type=int, default=400)
    ap.add_argument("--clicks", type=int, default=32)
    ap.add_argument("--radius", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    b, h, w = args.batch, args.height, args.width
    eng = get_engine("cuda")
    rng = np.random.default_rng(0)
    ids = (np.arange(h)[:, None] // 20) * (w // 20 + 1) + np.arange(w)[None, :] // 20          # 20x20 blocks: 300 regions
    seg1 = np.unique(ids, return_inverse=True)[1].reshape(h, w).astype(np.int32)
    n = int(seg1.max()) + 1
    seg = eng.to_device(np.broadcast_to(seg1, (b, h, w)).copy())
    node_ptr = eng.to_device(np.arange(b + 1, dtype=np.int32) * n)
    mask = eng.to_device(rng.integers(0, 4, (b, h, w)).astype(np.uint8))
    half = args.clicks // 2
    per_image = []
    for _ in range(b):
        pts = [(int(rng.integers(0, h)), int(rng.integers(0, w))) for _ in range(args.clicks)]
        per_image.append((pts[:half], pts[half:]))
    hints, hint_ptr = eng.upload_hints(*pack_hints(per_image))
    for region in (0, 1):
        for _ in range(3):
            eng.apply_hints(mask, hints, hint_ptr, args.radius, region, seg, node_ptr)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            eng.apply_hints(mask, hints, hint_ptr, args.radius, region, seg, node_ptr)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.reps
        print(f"region={region}: {ms:.3f} ms per call (host wall, {b} images {h}x{w}, {args.clicks} clicks each, "
              f"radius {args.radius})", flush=True)


if __name__ == "__main__":
    main()
