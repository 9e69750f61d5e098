"""experiment helper: ggc_trimap_matte at the defaults on batch 256 of 300x400 and batch 16 of 600x800, next to
ggc_closed_form_matte (the mask-band rows of DESIGN.md 5.13) on the same images in the same session.  The images are the
synthetic ones of tools/closed_form_rate.py; their GrabCut masks are feathered on the device (the guided matte) into a
stand-in true matte, and the trimap's unknown region is the Chebyshev dilation by k of its fractional pixels, as
tests/trimap_matte_ref.trimap_from_alpha, for k = 2 and k = 10.  Time per call from events over REPS calls after a warm-up,
iterations per image, and the share of 16 x 16 tiles the solver lists (tiles with U and their eight neighbours)."""
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
r, eps, band, max_iter, tol = cf.args()


def timed(fn):
    out = fn()                                                                  # warm-up (scratch)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS, out


def listed_share(unknown):
    """Share of the 16 x 16 tiles that hold an unknown pixel or touch a tile that does, over the images that are solved."""
    B, H, W = unknown.shape
    u = torch.nn.functional.max_pool2d(unknown[:, None].float(), 16, ceil_mode=True)
    near = torch.nn.functional.max_pool2d(u, 3, stride=1, padding=1)[:, 0]
    n = unknown.flatten(1).sum(1)
    solved = (n > 0) & (n < H * W)
    return (near[solved].sum() / near[0].numel() / B).item()


def report(what, ms, iters, rel, unknown):
    it = iters.cpu().numpy()
    print(f"{what}: {ms:.3f} ms per call; unknown {unknown.float().mean().item():.3f}; listed tiles "
          f"{listed_share(unknown):.3f}; iterations per image min {it.min()} median {int(np.median(it))} max {it.max()}; "
          f"rel_residual max {rel.max().item():.2e}", flush=True)


for B, H, W in ((256, 300, 400), (16, 600, 800)):
    imgs = np.stack([synthetic_image(H, W, 7000 + i % 16) for i in range(B)])
    bgr = eng.to_device(imgs)
    box = eng.to_device(np.broadcast_to(np.uint8(2), (B, H, W)).copy())         # GC_PR_BGD outside the box
    box[:, H // 8:H - H // 8, W // 8:W - W // 8] = 3                            # GC_PR_FGD inside
    mask = eng.grabcut(bgr, box, 5, 0, None, 0)[0].clone()
    alpha = eng.empty(B, H, W)
    ms, (_, iters, rel) = timed(lambda: eng.closed_form_matte(bgr, mask, r, eps, band, max_iter, tol, out=(alpha, None)))
    edge = torch.nn.functional.max_pool2d(mask[:, None].float(), 3, 1, 1) != -torch.nn.functional.max_pool2d(
        -mask[:, None].float(), 3, 1, 1)
    unknown = torch.nn.functional.max_pool2d(edge.float(), 2 * band + 1, 1, band)[:, 0] > 0
    report(f"closed_form_matte B={B} {H}x{W} {cf.args()}", ms, iters, rel, unknown)
    soft = eng.alpha_matte(bgr, mask, 4, 1e-4)                                  # the stand-in true matte
    frac = ((soft > 0) & (soft < 1))[:, None].float()
    for k in (2, 10):
        unknown = torch.nn.functional.max_pool2d(frac, 2 * k + 1, 1, k)[:, 0] > 0
        trimap = torch.where(unknown, torch.full_like(mask, 128), (soft >= 0.5).to(torch.uint8) * 255).contiguous()
        for start, a0 in (("0.5", None), ("mask", mask.float())):
            ms, (_, iters, rel) = timed(lambda: eng.trimap_matte(bgr, trimap, r, eps, max_iter, tol, alpha0=a0,
                                                                 out=(alpha, None)))
            report(f"trimap_matte B={B} {H}x{W} k={k} start {start} {(r, eps, max_iter, tol)}", ms, iters, rel, unknown)
