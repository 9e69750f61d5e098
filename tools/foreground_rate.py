"""experiment helper: ggc_estimate_foreground at the defaults on batch 256 of 300x400 and batch 16 of 600x800, synthetic
images, alpha from the closed-form matte of their GrabCut masks at its defaults (the inputs of tools/closed_form_rate.py);
time per call from events next to the closed-form matte's on the same inputs, iterations per image, listed tiles and
pixels of U.  MATTE=guided takes the guided matte's alpha instead.  Run it under `rocprofv3 --kernel-trace --stats` in a
run of its own for the per-kernel medians."""
import os
import sys
from pathlib import Path

root = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(root))
sys.path.insert(0, str(root / "src"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gcn_grabcut._engine import get_engine  # noqa: E402
from gcn_grabcut.pipeline import ClosedFormMatte, ForegroundColours  # noqa: E402
from gcn_grabcut.synthetic import synthetic_image  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
MATTE = os.environ.get("MATTE", "closed-form")
eng = get_engine("cuda")
cf, fgc = ClosedFormMatte(), ForegroundColours()


def timed(fn):
    fn()                                                                        # warm-up (scratch)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS, out


for B, H, W in ((256, 300, 400), (16, 600, 800)):
    imgs = np.stack([synthetic_image(H, W, 7000 + i % 16) for i in range(B)])
    bgr = eng.to_device(imgs)
    box = eng.to_device(np.broadcast_to(np.uint8(2), (B, H, W)).copy())         # GC_PR_BGD outside the box
    box[:, H // 8:H - H // 8, W // 8:W - W // 8] = 3                            # GC_PR_FGD inside
    mask = eng.grabcut(bgr, box, 5, 0, None, 0)[0].clone()
    alpha = eng.empty(B, H, W)
    if MATTE == "guided":
        ms_m, _ = timed(lambda: eng.alpha_matte(bgr, mask, 4, 1e-4, out=alpha))
        it_m = np.zeros(B, np.int64)
    else:
        ms_m, (_, it_m, _) = timed(lambda: eng.closed_form_matte(bgr, mask, *cf.args(), out=(alpha, None)))
        it_m = it_m.cpu().numpy()
    fg = eng.empty(B, H, W, 3, dtype=torch.uint8)
    ms, (_, iters, rel) = timed(lambda: eng.estimate_foreground(bgr, alpha, *fgc.args(), out=(fg, None)))
    it = iters.cpu().numpy()
    u = (alpha >= 1 / 510) & (alpha <= 1 - 1 / 510)
    n_u = int(u.sum().item())
    pad = (-H) % 16, (-W) % 16
    tiles = torch.nn.functional.pad(u, (0, pad[1], 0, pad[0])).view(B, (H + pad[0]) // 16, 16, (W + pad[1]) // 16, 16)
    n_tiles = int(tiles.any(4).any(2).sum().item())
    print(f"estimate_foreground B={B} {H}x{W} {fgc.args()} on the {MATTE} alpha: {ms:.3f} ms per call; |U| {n_u} pixels in "
          f"{n_tiles} listed tiles ({n_tiles * 256} listed pixels); iterations per image min {it.min()} median "
          f"{int(np.median(it))} max {it.max()}; rel_residual max {rel.max().item():.2e}; "
          f"{1e6 * ms / (max(int(it.max()), 1) * n_tiles * 256):.3f} ns per iteration (of the slowest image) and listed pixel", flush=True)
    print(f"  the {MATTE} matte on the same inputs: {ms_m:.3f} ms per call, iterations median {int(np.median(it_m))} max "
          f"{it_m.max()}", flush=True)
