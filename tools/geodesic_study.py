"""experiment helper: the study behind geodesic click hints.  Needs the MI355X.

    python3 tools/geodesic_study.py [--first-click] [--noc] [--time]        (no flag: all three)

Scenes are synthetic_image(H, W, 30000 + s, return_mask=True) for s = 0..7 at 120x160 (150 superpixels) and 300x400 (300
superpixels); the network is ResGCNNet(128, 6) with the seeded weights of tests/helpers.py (seed 0), so the automatic mask
is poor and the clicks have work to do.

  --first-click  the first simulated click of the NoC protocol on the automatic result (evaluate_clicks, max_clicks = 1),
                 painted as the r = 5 disk and as geodesic hints at a few (radius, gamma): pixels labelled, and pixels
                 labelled against the ground truth, summed over the eight scenes
  --noc          evaluate_clicks with 20 clicks: NoC@85, NoC@90, NoF@90 and the mean IoU after 1, 3, 5, 10 and 20 clicks
  --time         64 images of 300x400 with one foreground and one background click each (the centres of the ground truth's
                 and the background's distance transforms): ggc_geodesic_hints at the default settings, ggc_apply_hints
                 at r = 5 and one GC_EVAL GrabCut iteration on the same batch, by HIP events around the call on the
                 stream (3 warm-up calls, 20 timed, the median).  The geodesic call reads work-list lengths back, so its
                 time includes those synchronisations."""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "src"), str(ROOT / "tests")]

SETTINGS = [(20, 2), (40, 2), (40, 1), (40, 4), (60, 2)]                # (radius, gamma); (40, 2) is the default
SIZES = [(120, 160, 150), (300, 400, 300)]


def _pipeline(n_segments):
    from helpers import seeded_state_dict
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig
    model, _ = seeded_state_dict(128, 6, seed=0)
    return GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=n_segments), device="cuda")


def _scenes(h, w, n=8):
    from gcn_grabcut.synthetic import synthetic_image
    pairs = [synthetic_image(h, w, 30000 + s, return_mask=True) for s in range(n)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _wrong(lab, gt):
    return int(((lab == 1) & (gt == 0)).sum() + ((lab == 0) & (gt != 0)).sum())


def first_click():
    from gcn_grabcut import geodesic_hints
    print("size | hint | pixels labelled | labelled against the truth")
    for h, w, nseg in SIZES:
        imgs, gts = _scenes(h, w)
        clicks = _pipeline(nseg).evaluate_clicks(imgs, gts, max_clicks=1)["clicks"]
        yy, xx = np.mgrid[0:h, 0:w]
        tot = {("disk", 5, 0): [0, 0], **{("geodesic", r, g): [0, 0] for r, g in SETTINGS}}
        for img, gt, cl in zip(imgs, gts, clicks):
            if not cl:
                continue
            r0, c0, l0 = cl[0]
            disk = np.where((yy - r0) ** 2 + (xx - c0) ** 2 <= 25, l0, -1)
            tot[("disk", 5, 0)][0] += int((disk >= 0).sum())
            tot[("disk", 5, 0)][1] += _wrong(disk, gt)
            fg, bg = ([(r0, c0)], []) if l0 else ([], [(r0, c0)])
            for r, g in SETTINGS:
                m = geodesic_hints(img, fg, bg, r, g, mask=np.full((h, w), 255, np.uint8)).astype(np.int32)
                m[m == 255] = -1
                tot[("geodesic", r, g)][0] += int((m >= 0).sum())
                tot[("geodesic", r, g)][1] += _wrong(m, gt)
        for (kind, r, g), (n, bad) in tot.items():
            name = "disk r 5" if kind == "disk" else f"geodesic radius {r} gamma {g}"
            print(f"{h}x{w} | {name} | {n} | {bad}", flush=True)


def noc():
    from gcn_grabcut import GeodesicHints
    print("size | hint | NoC@85 | NoC@90 | NoF@90 | mIoU@1 | mIoU@3 | mIoU@5 | mIoU@10 | mIoU@20")
    for h, w, nseg in SIZES:
        imgs, gts = _scenes(h, w)
        pipe = _pipeline(nseg)
        for name, kw in [("disk r 5", dict(hint_radius=5))] + \
                        [(f"geodesic radius {r} gamma {g}", dict(geodesic=GeodesicHints(r, g))) for r, g in SETTINGS]:
            res = pipe.evaluate_clicks(imgs, gts, max_clicks=20, **kw)
            mi = res["mean_iou"]
            print(f"{h}x{w} | {name} | {res['noc'][0.85].mean():.2f} | {res['noc'][0.9].mean():.2f} | {res['nof'][0.9]} | " +
                  " | ".join(f"{mi[k]:.4f}" for k in (1, 3, 5, 10, 20)), flush=True)


def _median_ms(fn, warm=3, reps=20):
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


def timing():
    from scipy import ndimage
    from gcn_grabcut import GeodesicHints
    from gcn_grabcut.graph_builder import pack_hints
    from gcn_grabcut.synthetic import synthetic_image
    h, w, b = 300, 400, 64
    pipe = _pipeline(300)
    eng = pipe._eng
    pairs = [synthetic_image(h, w, 30000 + s, return_mask=True) for s in range(b)]

    def centre(region):
        e = ndimage.distance_transform_edt(np.pad(region, 1))[1:-1, 1:-1]
        return tuple(int(v) for v in np.unravel_index(e.argmax(), e.shape))

    per_image = [([centre(gt)], [centre(1 - gt)]) for _, gt in pairs]
    bgr = eng.to_device(np.stack([p[0] for p in pairs]))
    state = pipe.segment_batch_device(bgr, compose=False, return_state=True)
    hints, hint_ptr = eng.upload_hints(*pack_hints(per_image))
    g = GeodesicHints()
    mask = state["gc_mask"].clone()
    rows = [("ggc_geodesic_hints radius 40 gamma 2", lambda: eng.geodesic_hints(bgr, hints, hint_ptr, g.radius, g.gamma, mask=mask)),
            ("ggc_apply_hints r 5", lambda: eng.apply_hints(mask, hints, hint_ptr, 5)),
            ("one GC_EVAL iteration", lambda: eng.grabcut_lanes(state["gc_image"], state["gc_mask"].clone(), 1, 2, pipe.gc_config.seed,
                                                                 1, state["bgd"], state["fgd"]))]
    print(f"call | median ms | min | max   ({b} images {h}x{w}, one fg and one bg click each, HIP events, 3 warm-up + 20 calls)")
    for name, fn in rows:
        med, lo, hi = _median_ms(fn)
        print(f"{name} | {med:.3f} | {lo:.3f} | {hi:.3f}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--first-click", action="store_true")
    ap.add_argument("--noc", action="store_true")
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    every = not (a.first_click or a.noc or a.time)
    if a.first_click or every:
        first_click()
    if a.noc or every:
        noc()
    if a.time or every:
        timing()
