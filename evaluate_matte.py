"""
evaluate_matte.py — how good an alpha matte is: SAD, MSE, gradient and connectivity error against the true matte.

    python3 evaluate_matte.py --pred out/alphas --alphas data/alphas --trimaps data/trimaps
    python3 evaluate_matte.py --images data/images --masks data/masks --alphas data/alphas --method closed-form --cf-band 2
    python3 evaluate_matte.py --images imgs --masks masks --alphas gts --method guided --matte-radius 6 --json guided6.json
    python3 evaluate_matte.py --images data/images --trimaps data/trimaps --alphas data/alphas --method trimap

The four errors of Rhemann et al. (CVPR 2009) as the matting benchmarks report them, computed on the device
(gcn_grabcut.evaluate_matte).  Either --pred names a directory of saved mattes (8-bit, what
`inference.py --save alpha` writes), or --images and --masks name colour images and binary masks from which --method
makes the matte on the device: `mask` scores the hard mask itself, `guided` the guided-filter matte, `closed-form` the
closed-form matte.  `--method trimap` takes --images and --trimaps and no --masks: each image's matte is solved from its
trimap (255 foreground, 0 background, else unknown; gcn_grabcut.trimap_matte) and scored on that trimap's unknown
region.  Files are matched by stem with --alphas, the true mattes (8-bit grey).  With --trimaps only the pixels
whose trimap byte is neither 0 nor 255 are counted.  Images of one size are scored as one batch.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

EXTS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")
TAG = "[evaluate_matte]"


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Alpha-matte evaluation (SAD, MSE, Grad, Conn) of GCN-GrabCut (MI355X)")
    parser.add_argument("--alphas", required=True, help="Directory of true mattes (8-bit grey, same stem)")
    parser.add_argument("--pred", default=None, help="Directory of mattes to score (8-bit grey)")
    parser.add_argument("--images", default=None, help="Directory of colour images (with --masks and --method)")
    parser.add_argument("--masks", default=None, help="Directory of binary masks (> 127 = foreground)")
    parser.add_argument("--trimaps", default=None, help="Directory of trimaps: count only bytes that are neither 0 nor 255")
    parser.add_argument("--method", choices=["mask", "guided", "closed-form", "trimap"], default="guided",
                        help="How the matte is made from --images and --masks (trimap: from --images and --trimaps)")
    parser.add_argument("--matte-radius", type=int, default=4, help="Window radius of the guided matte, 1..64")
    parser.add_argument("--matte-eps", type=float, default=1e-4, help="Regularisation of the guided matte (>= 1e-12)")
    parser.add_argument("--cf-radius", type=int, default=1, help="Window radius of the closed-form matte, 1..8")
    parser.add_argument("--cf-eps", type=float, default=1e-5, help="Regularisation of the closed-form matte, [1e-12, 1]")
    parser.add_argument("--cf-band", type=int, default=1, help="Half-width of the unknown band around the mask's edge, 0..64")
    parser.add_argument("--cf-iters", type=int, default=500, help="Most conjugate-gradient iterations per image")
    parser.add_argument("--cf-tol", type=float, default=1e-4, help="Stop when the residual falls to this fraction")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--batch", type=int, default=64, help="Images per device batch")
    parser.add_argument("--json", default=None, help="Write per-image errors and their means here")
    return parser


def _by_stem(directory: str, what: str) -> dict:
    d = Path(directory)
    if not d.is_dir():
        raise SystemExit(f"{TAG} {what} directory {directory} does not exist")
    return {p.stem: p for p in sorted(d.iterdir()) if p.suffix.lower() in EXTS}


def _grey(path: Path) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("L"), dtype=np.uint8)


def _bgr(path: Path) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[:, :, ::-1])


def collect(args) -> list:
    """One dict per image: name, gt, and pred or image + mask, and region when --trimaps is given.  Every partner file
    must exist and have the true matte's size."""
    truth = _by_stem(args.alphas, "--alphas")
    dirs = {"pred": args.pred} if args.pred else {"image": args.images, "mask": args.masks}
    if args.method == "trimap" and not args.pred:
        del dirs["mask"]
    if args.trimaps:
        dirs["trimap"] = args.trimaps
    flags = {"pred": "--pred", "image": "--images", "mask": "--masks", "trimap": "--trimaps"}
    files = {k: _by_stem(v, flags[k]) for k, v in dirs.items()}
    first = files["pred"] if args.pred else files["image"]
    if not first:
        raise SystemExit(f"{TAG} no image files in {args.pred or args.images}")
    items = []
    for stem, path in first.items():
        if stem not in truth:
            raise SystemExit(f"{TAG} {path} has no true matte of the same stem in {args.alphas}")
        item = {"name": stem, "gt": _grey(truth[stem])}
        for kind, table in files.items():
            if stem not in table:
                raise SystemExit(f"{TAG} {path} has no {kind} of the same stem in {dirs[kind]}")
            a = _bgr(table[stem]) if kind == "image" else _grey(table[stem])
            if a.shape[:2] != item["gt"].shape:
                raise SystemExit(f"{TAG} {table[stem]} is {a.shape[1]}x{a.shape[0]} but the true matte {truth[stem]} is "
                                 f"{item['gt'].shape[1]}x{item['gt'].shape[0]}")
            item[kind] = a
        if "trimap" in item:
            t = item["trimap"]
            item["region"] = ((t != 0) & (t != 255)).astype(np.uint8)
        items.append(item)
    return items


def make_mattes(args, eng, images: np.ndarray, masks: np.ndarray):
    """(B,H,W) uint8 levels on the device of the chosen method's matte of masks (B,H,W) {0,1} under images; for the
    trimap method, masks holds the trimaps' bytes."""
    import torch
    m = eng.to_device(np.ascontiguousarray(masks))
    if args.method == "mask":
        return m * 255
    bgr = eng.to_device(np.ascontiguousarray(images))
    if args.method == "trimap":
        alpha = eng.trimap_matte(bgr, m, args.cf_radius, args.cf_eps, args.cf_iters, args.cf_tol)[0]
    elif args.method == "guided":
        alpha = eng.alpha_matte(bgr, m, args.matte_radius, args.matte_eps)
    else:
        alpha = eng.closed_form_matte(bgr, m, args.cf_radius, args.cf_eps, args.cf_band, args.cf_iters, args.cf_tol)[0]
    return torch.floor(alpha.double() * 255.0 + 0.5).to(torch.uint8)                 # pipeline.alpha_to_u8 on the device


def main() -> None:
    parser = build_parser()
    args = parser.parse_args()
    from_files = args.pred is not None
    from_masks = args.images is not None or args.masks is not None
    if from_files == from_masks:
        parser.error("give either --pred, or --images and --masks")
    by_trimap = from_masks and args.method == "trimap"
    if by_trimap and args.masks is not None:
        parser.error("--method trimap makes the matte from --images and --trimaps: drop --masks")
    if by_trimap and (args.images is None or args.trimaps is None):
        parser.error("--method trimap needs --images and --trimaps")
    if from_masks and not by_trimap and (args.images is None or args.masks is None):
        parser.error("--images and --masks go together")
    if args.batch < 1:
        parser.error("--batch must be >= 1")
    from src.gcn_grabcut._engine import check_closed_form_args, check_closed_form_shape, check_matte_args, get_engine
    from src.gcn_grabcut.metrics import matte_metrics_from_sums
    try:
        if from_masks and args.method == "guided":
            check_matte_args(args.matte_radius, args.matte_eps)
        if from_masks and args.method == "closed-form":
            check_closed_form_args(args.cf_radius, args.cf_eps, args.cf_band, args.cf_iters, args.cf_tol)
        if by_trimap:
            check_closed_form_args(args.cf_radius, args.cf_eps, 0, args.cf_iters, args.cf_tol)
    except ValueError as e:
        parser.error(str(e))

    items = collect(args)
    by_shape: dict = {}
    for it in items:
        by_shape.setdefault(it["gt"].shape, []).append(it)
    if from_masks and args.method in ("closed-form", "trimap"):
        for h, w in by_shape:
            try:
                check_closed_form_shape(h, w, args.cf_radius)
            except ValueError as e:
                raise SystemExit(f"{TAG} {e}")

    eng = get_engine(args.device)
    metrics = {}
    for items_s in by_shape.values():
        for i in range(0, len(items_s), args.batch):
            chunk = items_s[i:i + args.batch]
            gt = eng.to_device(np.stack([c["gt"] for c in chunk]))
            if from_files:
                pred = eng.to_device(np.stack([c["pred"] for c in chunk]))
            else:
                pred = make_mattes(args, eng, np.stack([c["image"] for c in chunk]),
                                   np.stack([c["trimap"] if by_trimap else (c["mask"] > 127).astype(np.uint8)
                                             for c in chunk]))
            region = eng.to_device(np.stack([c["region"] for c in chunk])) if args.trimaps else None
            sums, grad, _ = eng.matte_errors(pred, gt, region)
            sums, grad = sums.cpu().numpy(), grad.cpu().numpy()
            for j, c in enumerate(chunk):
                metrics[c["name"]] = matte_metrics_from_sums(sums[j], grad[j])

    names = [it["name"] for it in items]
    what = (f"mattes of {args.pred}" if from_files else f"trimap mattes of the trimaps of {args.trimaps}" if by_trimap
            else f"{args.method} mattes of the masks of {args.masks}")
    print(f"{TAG} {len(names)} image(s), {what}" + (", unknown region of the trimaps" if args.trimaps else ""))
    width = max(len(n) for n in names + ["mean"])
    print(f"  {'name':<{width}}  {'SAD':>10}  {'MSE':>12}  {'Grad':>10}  {'Conn':>10}  {'pixels':>9}")
    for n in names:
        m = metrics[n]
        print(f"  {n:<{width}}  {m.sad:>10.4f}  {m.mse:>12.6e}  {m.grad:>10.4f}  {m.conn:>10.4f}  {m.n_pixels:>9d}")
    mean = {k: float(np.mean([getattr(metrics[n], k) for n in names])) for k in ("sad", "mse", "grad", "conn")}
    print(f"  {'mean':<{width}}  {mean['sad']:>10.4f}  {mean['mse']:>12.6e}  {mean['grad']:>10.4f}  {mean['conn']:>10.4f}")

    if args.json:
        keys = ("method", "matte_radius", "matte_eps", "cf_radius", "cf_eps", "cf_band", "cf_iters", "cf_tol")
        doc = {"config": {"pred": args.pred, "alphas": args.alphas, "trimaps": args.trimaps,
                          **({} if from_files else {k: getattr(args, k) for k in keys})},
               "mean": mean, "images": [{"name": n, **metrics[n].as_dict()} for n in names]}
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
        print(f"{TAG} wrote {args.json}")


if __name__ == "__main__":
    sys.exit(main())
