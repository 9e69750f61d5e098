"""experiment helper: ggc_upsample_matte on a batch of 16 photos, 800x600 working -> 4000x3000 full (192 Mpx), every
output requested; device time per call from events, and the bytes model of stage 3 beside it.  Run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel split, then `--summarise <dir>` for the median
time of each of the three kernels and stage 3's share of the 6.29 TB/s measured copy rate."""
import glob
import os
import sys
from pathlib import Path

root = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(root))
sys.path.insert(0, str(root / "src"))

B = int(os.environ.get("B", "16"))
H, W = int(os.environ.get("H", "600")), int(os.environ.get("W", "800"))
H1, W1 = int(os.environ.get("H1", "3000")), int(os.environ.get("W1", "4000"))
REPS = int(os.environ.get("REPS", "10"))
COPY_TBS = 6.29
STAGE3_BYTES = 3 + 4 + 1 + 4          # per full pixel: BGR in; alpha f32, mask u8, BGRA out


def stage3_model():
    px = B * H1 * W1
    gb = px * STAGE3_BYTES / 1e9
    return px, gb, gb / COPY_TBS       # GB / (TB/s) = ms


def summarise(d: str) -> None:
    import csv
    import statistics
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    times: dict = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            if "k_matte_ab" in name or "k_matte_alpha" in name or "k_upsample" in name:
                times.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    px, gb, ms_model = stage3_model()
    for name, t in sorted(times.items()):
        med = statistics.median(t)
        line = f"{med:8.3f} ms median over {len(t):3d} calls  {name[:90]}"
        if "k_upsample" in name:
            line += f"  ({gb / med:.2f} TB/s, {ms_model / med:.0%} of {COPY_TBS} TB/s)"
        print(line)


def main() -> None:
    import numpy as np
    import torch
    from gcn_grabcut._engine import get_engine
    from gcn_grabcut.synthetic import synthetic_image
    eng = get_engine("cuda")
    pairs = [synthetic_image(H, W, 7100 + i, return_mask=True) for i in range(B)]
    bgr = eng.to_device(np.stack([p[0] for p in pairs]))
    mask = eng.to_device(np.stack([p[1] for p in pairs]))
    full = eng.empty(B, H1, W1, 3, dtype=torch.uint8)
    for i in range(B):                 # test input only: the working image enlarged on the device
        up = torch.nn.functional.interpolate(bgr[i:i + 1].permute(0, 3, 1, 2).float(), size=(H1, W1), mode="bilinear",
                                             align_corners=False)
        full[i] = up[0].permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8)
    out = (eng.empty(B, H1, W1), eng.empty(B, H1, W1, dtype=torch.uint8), eng.empty(B, H1, W1, 4, dtype=torch.uint8))
    px, gb, ms_model = stage3_model()
    print(f"stage 3 bytes model: {px / 1e6:.0f} Mpx x {STAGE3_BYTES} B = {gb:.2f} GB per call -> "
          f"{ms_model:.3f} ms at {COPY_TBS} TB/s", flush=True)
    for r in [int(v) for v in os.environ.get("RADII", "4,8").split(",")]:
        for _ in range(2):
            eng.upsample_matte(bgr, mask, full, r, 1e-4, out=out)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            eng.upsample_matte(bgr, mask, full, r, 1e-4, out=out)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / REPS
        print(f"upsample_matte B={B} {H}x{W} -> {H1}x{W1} r={r}: {ms:.3f} ms per call (three kernels)", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        main()
