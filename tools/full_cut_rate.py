"""experiment helper: the stages of the full-resolution banded cut on a batch of 16 photos, 1600x1200 from 400x300
(synthetic images, working mask = 4x4 box mean of the truth >= 0.5), HIP-event time per stage, median of REPS calls after
warm-up:

    lift          ggc_lift_labels (labels only), with its achieved GB/s against its byte model (1 B per pixel written,
                  plus 1/4 B per pixel of bit planes written and read back)
    lift (chain)  the same labels from existing entries: ggc_lift_trimap (the mask as trimap and as alpha), a threshold,
                  ggc_closed_form_band and a remap in torch; the baseline ggc_lift_labels must not be slower than
    colour        ggc_convert_color8 (lab)
    grabcut       ggc_grabcut(mode 0, 1 iteration) cold from the labels
    clean-up      ggc_clean_mask(0.002)
    compose       ggc_compose_outputs
    upsample_mask ggc_upsample_matte (alpha and mask, r 4, eps 1e-4) on the same batch, as context for the GrabCut stage

B, H1, W1, K (the reduction factor) and REPS come from the environment."""
import os
import sys
from pathlib import Path

root = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(root))
sys.path.insert(0, str(root / "src"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gcn_grabcut._engine import default_full_cut_band, get_engine  # noqa: E402
from gcn_grabcut.synthetic import synthetic_image  # noqa: E402

B, H1, W1, K = (int(os.environ.get(k, d)) for k, d in (("B", "16"), ("H1", "1200"), ("W1", "1600"), ("K", "4")))
REPS = max(10, int(os.environ.get("REPS", "10")))
H, W = H1 // K, W1 // K


def box_down(a):
    return np.asarray(a, np.float64).reshape(H, K, W, K, *a.shape[2:]).mean(axis=(1, 3))


def median_ms(fn, warm=2):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


eng = get_engine("cuda")
pairs = [synthetic_image(H1, W1, 31000 + i, return_mask=True) for i in range(min(B, 4))]
full = eng.to_device(np.stack([pairs[i % len(pairs)][0] for i in range(B)]))
work = eng.to_device(np.stack([np.rint(box_down(pairs[i % len(pairs)][0])).astype(np.uint8) for i in range(B)]))
mask = eng.to_device(np.stack([(box_down(pairs[i % len(pairs)][1] != 0) >= 0.5).astype(np.uint8) for i in range(B)]))
band = default_full_cut_band((H, W), (H1, W1))
px = B * H1 * W1
print(f"batch {B} x {H1}x{W1} from {H}x{W}, band {band}, median of {REPS} calls", flush=True)


def chain_labels():
    """The labels of ggc_lift_labels from the entries that existed before it."""
    _, a0 = eng.lift_trimap(mask * 255, mask.float(), (H1, W1), 0, want_trimap=False, want_alpha0=True)
    m1 = (a0 >= 0.5).to(torch.uint8)
    tri = eng.closed_form_band(m1, band)
    return torch.where(tri == 128, m1 | 2, m1)


labels, _ = eng.lift_labels(mask, (H1, W1), band)
same = bool(torch.equal(labels, chain_labels()))
t_lift = median_ms(lambda: eng.lift_labels(mask, (H1, W1), band))
t_chain = median_ms(chain_labels)
print(f"lift          {t_lift:9.3f} ms   {px / t_lift / 1e6:8.1f} GB/s of labels written, "
      f"{px * 1.5 / t_lift / 1e6:8.1f} GB/s with the bit planes (1 + 1/4 + 1/4 B per pixel)", flush=True)
print(f"lift (chain)  {t_chain:9.3f} ms   same labels: {same}   chain / lift = {t_chain / t_lift:.2f}", flush=True)
t_col = median_ms(lambda: eng.convert_color8(full, "lab"))
print(f"colour (lab)  {t_col:9.3f} ms", flush=True)
cut = {}


def grabcut():
    cut["binary"] = eng.grabcut(full, labels.clone(), 1, 0, None, 0)[0]


t_gc = median_ms(grabcut, warm=1)
t_clone = median_ms(lambda: labels.clone())
print(f"grabcut       {t_gc - t_clone:9.3f} ms   (1 iteration, cold; {t_clone:.3f} ms of label copy taken off)", flush=True)
cleaned = torch.empty_like(cut["binary"])
t_clean = median_ms(lambda: eng.clean_mask(cut["binary"], 0.002, False, out=cleaned))
print(f"clean-up      {t_clean:9.3f} ms", flush=True)
out = (eng.empty(B, H1, W1, 3, dtype=torch.uint8), eng.empty(B, H1, W1, 4, dtype=torch.uint8))
t_comp = median_ms(lambda: eng.compose(full, cleaned, out=out))
print(f"compose       {t_comp:9.3f} ms", flush=True)
up = (eng.empty(B, H1, W1), eng.empty(B, H1, W1, dtype=torch.uint8), None)
t_up = median_ms(lambda: eng.upsample_matte(work, mask, full, 4, 1e-4, out=up))
print(f"upsample_mask {t_up:9.3f} ms   (context: today's full mask)", flush=True)
