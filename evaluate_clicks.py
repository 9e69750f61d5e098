"""
evaluate_clicks.py — how well click guidance corrects the automatic mask, by the standard NoC protocol.

    python3 evaluate_clicks.py --images data/images --masks data/masks --checkpoint checkpoints/best_model.pt
    python3 evaluate_clicks.py --images imgs --masks gts --max-clicks 10 --targets 0.85 0.9 --json noc.json

A simulated user clicks the centre of the largest error region of every image, GrabCut continues from the edited mask,
and this repeats up to --max-clicks times (GCNGrabCutPipeline.evaluate_clicks).  Prints NoC@t (mean
clicks to reach IoU t), NoF@t (images that never reach it) and the mean IoU after 0, 1, 3, 5 and --max-clicks clicks;
--json writes every image's IoU curve and clicks.  Pairs are read as the training set is (dataset.list_image_mask_pairs /
materialise: same stem, --max-size resize, mask > 127); images of one size are evaluated as one batch.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Click-guidance evaluation (NoC protocol) of GCN-GrabCut (MI355X)")
    parser.add_argument("--images", required=True, help="Directory of images")
    parser.add_argument("--masks", required=True, help="Directory of ground-truth masks (same stem as the image)")
    parser.add_argument("--checkpoint", default="checkpoints/best_model.pt")
    parser.add_argument("--model", default="resgcn", choices=["resgcn", "gcn", "gat"])
    parser.add_argument("--hidden", type=int, default=128)
    parser.add_argument("--layers", type=int, default=6)
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--max-size", type=int, default=512, help="Shrink the longer side to this before segmenting")
    parser.add_argument("--superpixels", type=int, default=300)
    parser.add_argument("--batch", type=int, default=64, help="Images per device batch")
    parser.add_argument("--max-clicks", type=int, default=20)
    parser.add_argument("--targets", type=float, nargs="+", default=[0.85, 0.90], help="IoU targets of NoC / NoF")
    parser.add_argument("--hint-radius", type=int, default=5, help="Radius in pixels of the disk painted around a click")
    # additive: geodesic click hints (ggc_geodesic_hints) instead of disks
    parser.add_argument("--hint-mode", choices=["disk", "geodesic"], default="disk",
                        help="How a click is painted: a disk of --hint-radius, or the pixels within a geodesic distance of "
                             "it that does not cross colour edges (--geodesic-radius, --hint-gamma; --hint-radius is ignored)")
    parser.add_argument("--hint-gamma", type=int, default=2, help="Weight of the colour term of the geodesic distance, 0..64")
    parser.add_argument("--geodesic-radius", type=int, default=40,
                        help="Reach of a geodesic click over flat colour, in pixels of the image as segmented, 0..16384")
    parser.add_argument("--iters-per-click", type=int, default=1, help="GrabCut (GC_EVAL) iterations after each click")
    parser.add_argument("--stop-iou", type=float, default=None, help="No further clicks for an image at this IoU")
    parser.add_argument("--json", default=None, help="Write per-image curves and clicks here")
    return parser


def _check_sizes(pairs) -> None:
    """Refuses the run when an image and its mask differ in size (materialise would drop the pair silently)."""
    from PIL import Image
    for p in pairs:
        with Image.open(p["image_path"]) as im, Image.open(p["mask_path"]) as m:
            if im.size != m.size:
                raise SystemExit(f"[evaluate_clicks] {p['image_path']} is {im.size[0]}x{im.size[1]} but its mask "
                                 f"{p['mask_path']} is {m.size[0]}x{m.size[1]}")


def main() -> None:
    parser = build_parser()
    args = parser.parse_args()
    if args.max_clicks < 1:
        parser.error("--max-clicks must be >= 1")
    if args.iters_per_click < 1:
        parser.error("--iters-per-click must be >= 1")
    if args.hint_radius < 0:
        parser.error("--hint-radius must be >= 0")
    if not 0 <= args.hint_gamma <= 64:
        parser.error("--hint-gamma must be in 0..64")
    if not 0 <= args.geodesic_radius <= 16384:
        parser.error("--geodesic-radius must be in 0..16384")
    if args.batch < 1:
        parser.error("--batch must be >= 1")
    from inference import load_model
    from src.gcn_grabcut import GCNGrabCutPipeline, GeodesicHints
    from src.gcn_grabcut.dataset import list_image_mask_pairs, materialise
    from src.gcn_grabcut.graph_builder import SuperpixelGraphConfig
    from src.gcn_grabcut.metrics import noc_summary

    pairs = list_image_mask_pairs(args.images, args.masks, max_size=args.max_size)
    if not pairs:
        raise SystemExit(f"[evaluate_clicks] no image/mask pairs in {args.images} / {args.masks}")
    _check_sizes(pairs)
    model = load_model(args.checkpoint, args.model, args.hidden, args.layers, args.device, tag="evaluate_clicks")
    pipeline = GCNGrabCutPipeline(model, sp_config=SuperpixelGraphConfig(n_segments=args.superpixels), device=args.device)

    geodesic = GeodesicHints(args.geodesic_radius, args.hint_gamma) if args.hint_mode == "geodesic" else False
    by_shape: dict = {}
    for p in pairs:
        s = materialise(p)
        if s is None:
            print(f"[evaluate_clicks] skipping {p['image_path']}: unreadable, or a mask with under 200 pixels of a class")
            continue
        by_shape.setdefault(s["image"].shape, []).append(s)

    names, ious, clicks = [], [], []
    for items in by_shape.values():
        for i in range(0, len(items), args.batch):
            chunk = items[i:i + args.batch]
            r = pipeline.evaluate_clicks([s["image"] for s in chunk], [s["gt_mask"] for s in chunk],
                                         max_clicks=args.max_clicks, iou_targets=tuple(args.targets),
                                         hint_radius=args.hint_radius, iters_per_click=args.iters_per_click,
                                         stop_iou=args.stop_iou, geodesic=geodesic)
            names += [s["name"] for s in chunk]
            ious.append(r["ious"])
            clicks += r["clicks"]
            print(f"[evaluate_clicks] {len(names)} image(s) done, shape {chunk[0]['image'].shape[:2]}")
    if not names:
        raise SystemExit("[evaluate_clicks] nothing to evaluate")
    ious = np.concatenate(ious)
    summary = noc_summary(ious, args.targets, args.max_clicks)

    how = f"hint radius {args.hint_radius}" if not geodesic else \
        f"geodesic hints (radius {args.geodesic_radius}, gamma {args.hint_gamma})"
    print(f"\n[evaluate_clicks] {len(names)} image(s), up to {args.max_clicks} clicks, {how}, "
          f"{args.iters_per_click} GrabCut iteration(s) per click")
    for t in summary["noc"]:
        print(f"  NoC@{t:.2f} = {summary['noc'][t].mean():.2f}   NoF@{t:.2f} = {summary['nof'][t]}")
    ks = sorted({k for k in (0, 1, 3, 5, args.max_clicks) if k <= args.max_clicks})
    print("  mIoU  " + "  ".join(f"@{k}={summary['mean_iou'][k]:.4f}" for k in ks))

    if args.json:
        doc = {
            "config": {k: getattr(args, k) for k in ("max_clicks", "targets", "hint_radius", "hint_mode", "hint_gamma",
                                                      "geodesic_radius", "iters_per_click", "stop_iou",
                                                      "superpixels", "max_size", "checkpoint", "model")},
            "noc": {f"{t:.2f}": float(summary["noc"][t].mean()) for t in summary["noc"]},
            "nof": {f"{t:.2f}": summary["nof"][t] for t in summary["nof"]},
            "mean_iou": [float(v) for v in summary["mean_iou"]],
            "images": [{"name": n, "ious": [float(v) for v in ious[i]],
                        "noc": {f"{t:.2f}": int(summary["noc"][t][i]) for t in summary["noc"]},
                        "clicks": [list(c) for c in clicks[i]]} for i, n in enumerate(names)],
        }
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
        print(f"[evaluate_clicks] wrote {args.json}")


if __name__ == "__main__":
    sys.exit(main())
