"""Cost of the magic wand (ggc_wand_select) on the benchmark's batch and on one large image.

    python3 tools/wand_cost.py                  every step below as a child process under its own time limit; stops at the
                                                first step that fails or runs out of time
    python3 tools/wand_cost.py --step bench     256 images of 400x300 (the bench scenes): 1, 3 and 8 seeds per image at
                                                connectivity 8 and 0
    python3 tools/wand_cost.py --step large     one 1200x1600 image, 1 seed, connectivity 8 and 0

Timed by HIP events around the call on the stream, 3 warm-up + 20 calls, median (min-max); the per-kernel split comes from
ggc_profile_query on one more call.  The call synchronises the stream twice (it reads the seeds back and uploads the table
of live seeds), so the event time holds those two round trips.

The yardstick is a streaming floor: the bytes a call MUST move divided by the rate a device-to-device copy of 256 MiB reaches
in the same run (read + write counted).  Per pixel, with S seeds per image, contiguous: init reads 3 B of bgr and writes 4 B
per seed, merge reads 4 B per seed, compress reads and writes 4 B per seed, decide reads 4 B per seed and writes 1 B, emit
reads 1 B and writes select (1 B): 20 S + 3 S + 3 bytes.  Not contiguous: 3 B of bgr read, 1 B written.  The bench batch's
maps fit the 256 MiB last-level cache only for S = 1 (123 MB), so a call can beat the floor there; it is a yardstick for
"how many passes over the data does this cost", not a bound."""
import argparse
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "src")]

SCOPES = ("wand_refs", "wand_init", "wand_merge", "wand_compress", "wand_decide", "wand_emit", "wand_similar")
STEPS = {"bench": 420, "large": 180}        # seconds each may take


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


def copy_rate():
    """Bytes per second, read + write, of a device-to-device copy of 256 MiB in this run."""
    import torch
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    med, _, _ = median_ms(lambda: dst.copy_(src))
    return 2 * src.numel() / (med * 1e-3)


def seeds_for(h, w, per_image, b):
    """per_image seeds per image on a fixed lattice, labels alternating: the same for every image."""
    pts = [((2 * k + 1) * h // (2 * per_image), ((7 * k + 3) % per_image * 2 + 1) * w // (2 * per_image)) for k in range(per_image)]
    rows = np.array([[r, c, (k + 1) % 2] for _ in range(b) for k, (r, c) in enumerate(pts)], np.int32)
    return rows, np.arange(b + 1, dtype=np.int32) * per_image


def report(eng, name, bgr, per_image, conn, rate, tolerance=32):
    import torch
    b, h, w, _ = bgr.shape
    rows, ptr = seeds_for(h, w, per_image, b)
    d_rows, d_ptr = eng.upload_hints(rows, ptr)
    sel = torch.empty((b, h, w), dtype=torch.uint8, device="cuda")
    cnt = torch.empty((b, 2), dtype=torch.int32, device="cuda")

    def fn():
        eng.ctx.call("ggc_wand_select", eng._stream(), b, h, w, bgr.data_ptr(), d_rows.data_ptr(), d_ptr.data_ptr(), tolerance, conn,
                     1, None, sel.data_ptr(), cnt.data_ptr())

    med, lo, hi = median_ms(fn)
    eng.ctx.profile_enable(1)
    fn()
    split = {s: eng.ctx.profile_query(s) for s in SCOPES}
    eng.ctx.profile_enable(0)
    n = b * h * w
    must = n * ((20 + 3) * per_image + 3) if conn else n * 4
    floor = 1e3 * must / rate
    picked = float((sel != 0).float().mean().item())
    parts = " ".join(f"{s[5:]}={ms:.3f}x{k}" for s, (k, ms) in split.items() if k)
    print(f"{name} | {per_image} | {conn} | {med:.3f} | {lo:.3f} | {hi:.3f} | {floor:.3f} | {med / floor:.1f} | {100 * picked:.1f} % | {parts}",
          flush=True)


def step(name):
    from gcn_grabcut._engine import get_engine
    from gcn_grabcut.synthetic import synthetic_image
    eng = get_engine("cuda")
    rate = copy_rate()
    print(f"## step {name}: device copy of 256 MiB at {rate / 1e12:.2f} TB/s (read + write)", flush=True)
    print("batch | seeds per image | connectivity | median ms | min | max | floor ms | median / floor | selected | kernels ms x launches",
          flush=True)
    if name == "bench":
        bgr = eng.to_device(np.stack([synthetic_image(300, 400, 30000 + i) for i in range(256)]))
        for conn in (8, 0):
            for per_image in (1, 3, 8):
                report(eng, "256 x 400x300", bgr, per_image, conn, rate)
    else:
        small = synthetic_image(300, 400, 30000)
        big = np.ascontiguousarray(np.kron(small, np.ones((4, 4, 1), np.uint8)))       # 1200 x 1600: the scene, every pixel a 4x4 block
        bgr = eng.to_device(big[None])
        for conn in (8, 0):
            report(eng, "1 x 1600x1200", bgr, 1, conn, rate)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    args = ap.parse_args()
    if args.step:
        return step(args.step)
    for name, limit in STEPS.items():                                                   # nothing is started after a failure
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--step", name], timeout=limit)
        if r.returncode != 0:
            raise SystemExit(f"step {name} failed with status {r.returncode}: stopping")


if __name__ == "__main__":
    main()
