"""experiment helper: ggc_closed_form_matte at the defaults on batch 256 of 300x400 and batch 16 of 600x800, synthetic
images and their GrabCut masks; time per call from events, iterations per image, and the bytes model of DESIGN.md 5.13.
Run it under `rocprofv3 --kernel-trace --stats` in a run of its own for the per-kernel medians."""
import os
import sys
from pathlib import Path

root = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(root))
sys.path.insert(0, str(root / "src"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gcn_grabcut._engine import get_engine  # noqa: E402
from gcn_grabcut.pipeline import ClosedFormMatte  # noqa: E402
from gcn_grabcut.synthetic import synthetic_image  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
eng = get_engine("cuda")
cf = ClosedFormMatte()
for B, H, W in ((256, 300, 400), (16, 600, 800)):
    imgs = np.stack([synthetic_image(H, W, 7000 + i % 16) for i in range(B)])
    bgr = eng.to_device(imgs)
    box = eng.to_device(np.broadcast_to(np.uint8(2), (B, H, W)).copy())         # GC_PR_BGD outside the box
    box[:, H // 8:H - H // 8, W // 8:W - W // 8] = 3                            # GC_PR_FGD inside
    mask = eng.grabcut(bgr, box, 5, 0, None, 0)[0].clone()
    alpha = eng.empty(B, H, W)
    eng.closed_form_matte(bgr, mask, *cf.args(), out=(alpha, None))             # warm-up (scratch)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        _, iters, rel = eng.closed_form_matte(bgr, mask, *cf.args(), out=(alpha, None))
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / REPS
    it = iters.cpu().numpy()
    fg = mask.float().mean().item()
    print(f"closed_form_matte B={B} {H}x{W} {cf.args()}: {ms:.3f} ms per call; fg {fg:.3f}; iterations per image "
          f"min {it.min()} median {int(np.median(it))} max {it.max()}; rel_residual max {rel.max().item():.2e}", flush=True)
