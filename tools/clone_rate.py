"""experiment helper: ggc_poisson_clone (source and mixed gradients) and ggc_composite_over at batch 1, 16 and 256 of
300x400 synthetic images, an elliptic object mask of a quarter of the frame pasted at (0, 0) of another synthetic image;
time per call from events, iterations per image, listed tiles, and the bytes the solve's two tile kernels move per
iteration against the HBM peak.  Run it under `rocprofv3 --kernel-trace --stats` in a run of its own for the per-kernel
medians."""
import os
import sys
from pathlib import Path

root = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(root))
sys.path.insert(0, str(root / "src"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gcn_grabcut._engine import get_engine  # noqa: E402
from gcn_grabcut.pipeline import Clone  # noqa: E402
from gcn_grabcut.synthetic import synthetic_image  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
HBM_PEAK = 8.0e12                                 # bytes per second, the part's specification
# per pixel of Omega and iteration: k_cgc_apply<CloneProblem> reads r and the old p and writes the new p and q (4 x 24
# bytes); k_cgc_update<CloneProblem> reads p, q, x, r and writes x, r (6 x 24 bytes).  Per listed pixel: the byte plane, staged with its halo
# by the first and read once by the second (324 / 256 + 1 bytes).  The halo's r and p (68 entries a tile at most, held by
# neighbour tiles that read them too) are left out.
BYTES_OMEGA, BYTES_LISTED = 240.0, 324.0 / 256.0 + 1.0
eng = get_engine("cuda")
H, W = 300, 400


def timed(fn):
    fn()                                                                        # warm-up (scratch, code objects)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS, out


y, x = np.mgrid[:H, :W]
ellipse = ((((y - H / 2) / (0.282 * H)) ** 2 + ((x - W / 2) / (0.282 * W)) ** 2) <= 1.0).astype(np.uint8)
for B in (1, 16, 256):
    src = eng.to_device(np.stack([synthetic_image(H, W, 7000 + i % 16) for i in range(B)]))
    tgt = eng.to_device(np.stack([synthetic_image(H, W, 7100 + i % 16) for i in range(B)]))
    mask = eng.to_device(np.broadcast_to(ellipse, (B, H, W)).copy())
    off = np.zeros((B, 2), np.int32)
    padded = np.pad(ellipse, ((0, (-H) % 16), (0, (-W) % 16)))
    tiles = int(padded.reshape(padded.shape[0] // 16, 16, padded.shape[1] // 16, 16).any(3).any(1).sum()) * B
    for mixed in (False, True):
        clone = Clone(mixed=mixed)
        ms, (_, n, iters, rel) = timed(lambda: eng.poisson_clone(src, mask, tgt, off, *clone.args()))
        it, n_om = iters.cpu().numpy(), int(n.sum().item())
        per_iter = BYTES_OMEGA * n_om + BYTES_LISTED * 256 * tiles
        floor_ms = 1e3 * per_iter * int(it.max()) / HBM_PEAK
        print(f"poisson_clone B={B} {H}x{W} {clone.args()}: {ms:.3f} ms per call; |Omega| {n_om} pixels "
              f"({n_om / (B * H * W):.1%} of the frame) in {tiles} listed tiles; iterations per image min {it.min()} median "
              f"{int(np.median(it))} max {it.max()}; rel_residual max {rel.max().item():.2e}; {per_iter / 1e6:.2f} MB per "
              f"iteration, {per_iter * int(it.max()) / 1e9:.2f} GB per call = {floor_ms:.3f} ms at the HBM peak "
              f"({floor_ms / ms:.1%} of the call); {1e3 * ms / max(int(it.max()), 1):.2f} us per iteration", flush=True)
    rgba = torch.cat([src, (mask * 255)[..., None]], dim=3).contiguous()
    out = eng.empty(B, H, W, 3, dtype=torch.uint8)
    ms, _ = timed(lambda: eng.composite_over(rgba, tgt, off, out=out))
    moved = B * H * W * (4 + 3 + 3)
    print(f"composite_over B={B} {H}x{W}: {ms:.4f} ms per call; {moved / 1e6:.2f} MB moved = "
          f"{1e3 * moved / HBM_PEAK:.4f} ms at the HBM peak ({1e3 * moved / HBM_PEAK / ms:.1%} of the call)", flush=True)
