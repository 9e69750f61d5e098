"""experiment helper: the study behind intelligent scissors.

    python3 tools/scissors_study.py [--table] [--time]        (no flag: both; --time needs the MI355X)

  --table  CPU only, from the definition's restatement (tests/scissors_ref.py): the eight scenes
           synthetic_image(120, 160, 30000..30007, return_mask=True), 4 / 6 / 8 anchors taken from the ground truth's outline
           (scissors_ref.boundary_anchors), the defaults margin 16, edge_cap 2048, smooth 16.  Mean and worst distance, in
           pixels, of the traced path's pixels and of the straight chords' pixels to the true boundary.
  --time   64 images of 300x400 (scenes 30000..30063) with one closed 8-anchor path each, at the defaults: ggc_trace_paths
           (filling call with the capacity known, and the count-only call), ggc_apply_polygons on the traced lassos and one
           GC_EVAL GrabCut iteration on the same batch, by HIP events around the call on the stream (3 warm-up calls, 20 timed,
           the median).  Then one profiled call split into guide, relaxation rounds and walk by ggc_profile_query, with the
           number of rounds and the longest walk.  ggc_trace_paths reads its inputs, work-list lengths and totals back, so its
           time includes those synchronisations."""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "src"), str(ROOT / "tests")]


def table():
    import scissors_ref as ref
    print("anchors | traced mean | chords mean | ratio | traced worst pixel | chords worst pixel")
    for n, tm, cm, tw, cw in ref.study_rows():
        print(f"{n} | {tm:.2f} | {cm:.2f} | {tm / cm:.2f} | {tw:.1f} | {cw:.1f}", flush=True)


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


def _walk_lengths(verts, anchors):
    """Steps of each segment of one closed path: a segment ends the first time its walk reaches the next anchor."""
    out, start, k = [], 0, 1
    for i, v in enumerate(verts):
        if k < len(anchors) and i > start and tuple(v) == tuple(anchors[k]):
            out.append(i - start)
            start, k = i, k + 1
    out.append(len(verts) - start)
    return out


def timing():
    import torch
    import scissors_ref as ref
    from helpers import seeded_state_dict
    from gcn_grabcut import GCNGrabCutPipeline, Scissors, SuperpixelGraphConfig
    from gcn_grabcut.graph_builder import pack_paths
    from gcn_grabcut.synthetic import synthetic_image
    h, w, b = 300, 400, 64
    model, _ = seeded_state_dict(128, 6, seed=0)
    pipe = GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=300), device="cuda")
    eng = pipe._eng
    pairs = [synthetic_image(h, w, 30000 + s, return_mask=True) for s in range(b)]
    anchors = [ref.boundary_anchors(gt, 8)[1] for _, gt in pairs]
    bgr = eng.to_device(np.stack([p[0] for p in pairs]))
    state = pipe.segment_batch_device(bgr, compose=False, return_state=True)
    opt = Scissors()
    packed = pack_paths([[a] for a in anchors])
    d = eng.upload_paths(*packed)
    verts, vert_ptr = eng.trace_paths(bgr, *d, opt.margin, opt.edge_cap, opt.smooth)
    n = int(verts.size(0))
    labels = torch.full((b,), 2, dtype=torch.int32, device=eng.device)
    mask = state["gc_mask"].clone()
    rows = [("ggc_trace_paths, filling call", lambda: eng.trace_paths(bgr, *d, opt.margin, opt.edge_cap, opt.smooth, capacity=n)),
            ("ggc_trace_paths, count only", lambda: eng.ctx.call(
                "ggc_trace_paths", eng._stream(), b, h, w, bgr.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                d[3].data_ptr(), b, opt.margin, opt.edge_cap, opt.smooth, vert_ptr.data_ptr(), None, 0)),
            ("ggc_apply_polygons on the traced lassos", lambda: eng.apply_polygons(mask, verts, vert_ptr, labels, d[3])),
            ("one GC_EVAL iteration", lambda: eng.grabcut_lanes(state["gc_image"], state["gc_mask"].clone(), 1, 2, pipe.gc_config.seed,
                                                                 1, state["bgd"], state["fgd"]))]
    print(f"call | median ms | min | max   ({b} images {h}x{w}, one closed 8-anchor path each, {n} traced vertices, HIP events, "
          "3 warm-up + 20 calls)")
    for name, fn in rows:
        med, lo, hi = _median_ms(fn)
        print(f"{name} | {med:.3f} | {lo:.3f} | {hi:.3f}", flush=True)
    eng.ctx.profile_enable(1)
    eng.trace_paths(bgr, *d, opt.margin, opt.edge_cap, opt.smooth, capacity=n)
    print("part of one filling call | launches | total ms   (HIP events around each launch)")
    for name in ("scissors_guide", "scissors_round", "scissors_walk"):
        launches, ms = eng.ctx.profile_query(name)
        print(f"{name} | {launches} | {ms:.3f}", flush=True)
    eng.ctx.profile_enable(0)
    vp, v = vert_ptr.cpu().numpy(), verts.cpu().numpy()
    walks = [s for i in range(b) for s in _walk_lengths(v[vp[i]:vp[i + 1]], anchors[i])]
    area = sum(ref.window(p, q, opt.margin, h, w)[2] * ref.window(p, q, opt.margin, h, w)[3] for a in anchors for p, q in ref.segments(a, True))
    print(f"segments {len(walks)} | window pixels {area} | longest walk {max(walks)} steps | mean walk {np.mean(walks):.1f} steps")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    every = not (a.table or a.time)
    if a.table or every:
        table()
    if a.time or every:
        timing()
