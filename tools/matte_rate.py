"""experiment helper: ggc_alpha_matte on the bench-sized batch (256 x 300 x 400, synthetic images and their masks), device
time per call from events; run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split"""
import os
import sys
from pathlib import Path

root = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(root))
sys.path.insert(0, str(root / "src"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gcn_grabcut._engine import get_engine  # noqa: E402
from gcn_grabcut.synthetic import synthetic_image  # noqa: E402

B, H, W = int(os.environ.get("B", "256")), int(os.environ.get("H", "300")), int(os.environ.get("W", "400"))
REPS = int(os.environ.get("REPS", "20"))
eng = get_engine("cuda")
pairs = [synthetic_image(H, W, 7000 + i, return_mask=True) for i in range(16)]
bgr = eng.to_device(np.stack([pairs[i % 16][0] for i in range(B)]))
mask = eng.to_device(np.stack([pairs[i % 16][1] for i in range(B)]))
alpha = eng.empty(B, H, W)
for r in [int(v) for v in os.environ.get("RADII", "4,8").split(",")]:
    for _ in range(3):
        eng.alpha_matte(bgr, mask, r, 1e-4, out=alpha)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        eng.alpha_matte(bgr, mask, r, 1e-4, out=alpha)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / REPS
    print(f"alpha_matte B={B} {H}x{W} r={r}: {ms:.3f} ms per call ({B * H * W / ms / 1e6:.2f} Gpx/s)", flush=True)
