"""
matte.py — alpha mattes from images and trimaps with the closed-form matte on MI355X.  No segmentation is run.

    python3 matte.py --image cat.jpg --trimap cat_trimap.png
    python3 matte.py --input data/images --trimaps data/trimaps --output mattes/ --save alpha cutout
    python3 matte.py --image cat.jpg --trimap cat_trimap.png --save cutout --decontaminate
    python3 matte.py --image cat_small.jpg --trimap cat_small_trimap.png --full-image cat.jpg   # solved at cat.jpg's size
    python3 matte.py --image cat.jpg --mask cat_mask.png --band 3:5     # the trimap is made from a mask: unknown within 3 px inside, 5 outside

A trimap is an 8-bit grey image of the photo's size: 255 = foreground, 0 = background, every other byte unknown (the
convention of the matting benchmarks and of evaluate_matte.py --trimaps).  The matting Laplacian is solved on the
unknown pixels (gcn_grabcut.trimap_matte, ggc_trimap_matte).  With --input, trimaps are matched by stem;
images of one size are solved as one batch.  Outputs are named as inference.py names them: <stem>_alpha.png (8-bit grey)
and <stem>_cutout.png (BGRA cut-out with that alpha).

With --mask and --band INNER[:OUTER] instead of --trimap, the trimap is made on the device from a binary mask (any nonzero
byte foreground, for instance inference.py's <stem>_mask.png): foreground further than INNER pixels from the background
stays 255, background further than OUTER (default INNER) from the foreground stays 0, the band between is unknown
(gcn_grabcut.mask_to_trimap, ggc_modify_mask).

With --full-image (or --full-images DIR, matched by stem) the image and trimap are the working-size version of a larger
photo: the matte is solved at the working size, lifted, and solved again on the larger photo from there
(gcn_grabcut.trimap_matte_full), and the outputs have the larger photo's size.
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

IMAGE_EXTS = {".jpg", ".jpeg", ".png", ".bmp", ".tif", ".tiff", ".webp"}
TAG = "[matte]"


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Closed-form alpha mattes from images and trimaps (MI355X)")
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument("--image", help="Path to a single input image (with --trimap)")
    src.add_argument("--input", help="Directory of images (with --trimaps)")
    parser.add_argument("--trimap", default=None, help="Trimap of --image: 255 foreground, 0 background, else unknown")
    parser.add_argument("--trimaps", default=None, help="Directory of trimaps of --input, matched by stem")
    parser.add_argument("--mask", default=None,
                        help="Instead of --trimap: a binary mask of --image (any nonzero byte foreground); goes with --band")
    parser.add_argument("--band", default=None, metavar="INNER[:OUTER]",
                        help="With --mask: the unknown band around the mask's boundary, INNER pixels into the foreground "
                             "and OUTER (default INNER) into the background, by exact Euclidean distance")
    parser.add_argument("--output", default="results", help="Output directory")
    parser.add_argument("--save", nargs="+", default=["alpha"], choices=["alpha", "cutout"],
                        help="Which outputs to write: the matte, the BGRA cut-out with it")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--batch", type=int, default=64, help="Images per device batch")
    parser.add_argument("--cf-radius", type=int, default=1, help="Window radius of the closed-form matte, 1..8")
    parser.add_argument("--cf-eps", type=float, default=1e-5, help="Regularisation of the closed-form matte, [1e-12, 1]")
    parser.add_argument("--cf-iters", type=int, default=500, help="Most conjugate-gradient iterations per image")
    parser.add_argument("--cf-tol", type=float, default=1e-4, help="Stop when the residual falls to this fraction")
    parser.add_argument("--full-image", default=None,
                        help="The photo of --image at a larger size: solve there too, from the working-size matte")
    parser.add_argument("--full-images", default=None, help="Directory of larger versions of --input, matched by stem")
    parser.add_argument("--cf-grow", type=int, default=0,
                        help="With a full image: pixels of its size the lifted unknown region is grown by, 0..64")
    parser.add_argument("--cf-full-iters", type=int, default=2000,
                        help="With a full image: most conjugate-gradient iterations per image at its size")
    parser.add_argument("--decontaminate", action="store_true",
                        help="Write the cut-out (--save cutout) with estimated foreground colours where alpha is "
                             "fractional, instead of the image's own, so that it shows no halo on a new background")
    return parser


def _read(path: Path, mode: str):
    from PIL import Image
    try:
        with Image.open(path) as im:
            a = np.asarray(im.convert(mode), dtype=np.uint8)
    except Exception:
        raise SystemExit(f"{TAG} cannot read {path}")
    return np.ascontiguousarray(a[:, :, ::-1]) if mode == "RGB" else np.ascontiguousarray(a)


def collect(args) -> list:
    """(image path, trimap path, full image path or None) triples."""
    if args.image:
        pairs = [(Path(args.image), Path(args.trimap or args.mask), Path(args.full_image) if args.full_image else None)]
    else:
        in_dir, tri_dir = Path(args.input), Path(args.trimaps)
        for d, flag in ((in_dir, "--input"), (tri_dir, "--trimaps")):
            if not d.is_dir():
                raise SystemExit(f"{TAG} {flag} directory {d} does not exist")
        tris = {p.stem: p for p in sorted(tri_dir.iterdir()) if p.suffix.lower() in IMAGE_EXTS}
        images = sorted(p for p in in_dir.iterdir() if p.suffix.lower() in IMAGE_EXTS)
        if not images:
            raise SystemExit(f"{TAG} no image files in {in_dir}")
        for p in images:
            if p.stem not in tris:
                raise SystemExit(f"{TAG} {p} has no trimap of the same stem in {tri_dir}")
        fulls = {}
        if args.full_images:
            full_dir = Path(args.full_images)
            if not full_dir.is_dir():
                raise SystemExit(f"{TAG} --full-images directory {full_dir} does not exist")
            fulls = {p.stem: p for p in sorted(full_dir.iterdir()) if p.suffix.lower() in IMAGE_EXTS}
            for p in images:
                if p.stem not in fulls:
                    raise SystemExit(f"{TAG} {p} has no full image of the same stem in {full_dir}")
        pairs = [(p, tris[p.stem], fulls.get(p.stem)) for p in images]
    for p, t, full in pairs:
        for f in (p, t) if full is None else (p, t, full):
            if not f.is_file():
                raise SystemExit(f"{TAG} {f} does not exist")
    return pairs


def main() -> None:
    parser = build_parser()
    args = parser.parse_args()
    if args.image and ((args.trimap is None) == (args.mask is None) or args.trimaps is not None):
        parser.error("--image goes with --trimap (one file) or with --mask and --band, not --trimaps")
    if (args.mask is None) != (args.band is None) or (args.mask is not None and not args.image):
        parser.error("--mask and --band go together, with --image")
    if args.input and (args.trimaps is None or args.trimap is not None):
        parser.error("--input goes with --trimaps (a directory), not --trimap")
    if args.image and args.full_images is not None:
        parser.error("--image goes with --full-image (one file), not --full-images")
    if args.input and args.full_image is not None:
        parser.error("--input goes with --full-images (a directory), not --full-image")
    if args.decontaminate and "cutout" not in args.save:
        parser.error("--decontaminate changes the cut-out: add cutout to --save")
    if args.batch < 1:
        parser.error("--batch must be >= 1")
    from src.gcn_grabcut._engine import (check_closed_form_args, check_closed_form_shape, check_lift_args, get_engine)
    from src.gcn_grabcut.pipeline import ForegroundColours, ModifyMask, _write_png, alpha_to_u8
    band = None
    if args.band is not None:
        try:
            radii = [float(t) for t in args.band.split(":")]
            if len(radii) not in (1, 2):
                raise ValueError(f"--band takes INNER or INNER:OUTER, got {args.band!r}")
            band = ModifyMask("trimap", radii[0], radii[1] if len(radii) == 2 else None).args()
        except ValueError as e:
            parser.error(str(e))
    cf = (args.cf_radius, args.cf_eps, args.cf_iters, args.cf_tol)
    try:
        check_closed_form_args(cf[0], cf[1], 0, cf[2], cf[3])
        check_closed_form_args(cf[0], cf[1], 0, args.cf_full_iters, cf[3])
        check_lift_args((1, 1, 1), None, (1, 1), args.cf_grow)
    except ValueError as e:
        parser.error(str(e))

    by_shape: dict = {}
    for path, tri, full_path in collect(args):
        image, trimap = _read(path, "RGB"), _read(tri, "L")
        full = None if full_path is None else _read(full_path, "RGB")
        if trimap.shape != image.shape[:2]:
            raise SystemExit(f"{TAG} {tri} is {trimap.shape[1]}x{trimap.shape[0]} but {path} is "
                             f"{image.shape[1]}x{image.shape[0]}")
        try:
            check_closed_form_shape(*image.shape[:2], cf[0])
        except ValueError as e:
            raise SystemExit(f"{TAG} {path}: {e}")
        if full is not None:
            try:
                check_lift_args((1, *trimap.shape), None, full.shape[:2], args.cf_grow)
            except ValueError as e:
                raise SystemExit(f"{TAG} {full_path}: {e}")
        by_shape.setdefault((image.shape, None if full is None else full.shape), []).append((path, image, trimap, full))

    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{TAG} no MI355X visible: this build has no CPU path")
    eng = get_engine(args.device)
    out_dir = Path(args.output)
    out_dir.mkdir(parents=True, exist_ok=True)
    n_all, n_done, total_t = sum(len(v) for v in by_shape.values()), 0, 0.0
    for items in by_shape.values():
        for i in range(0, len(items), args.batch):
            chunk = items[i:i + args.batch]
            t0 = time.perf_counter()
            bgr = eng.to_device(np.stack([im for _, im, _, _ in chunk]))
            tri = eng.to_device(np.stack([t for _, _, t, _ in chunk]))
            if band is not None:                          # --mask: the trimap is made here, from the mask that was read
                tri = eng.modify_mask(tri, *band)
                chunk = [(p, im, t, f) for (p, im, _, f), t in zip(chunk, tri.cpu().numpy())]
            if chunk[0][3] is None:
                alpha, rgba, iters, rel = eng.trimap_matte(bgr, tri, *cf, want_rgba=True)
            else:                                         # the working-size solve, the lift, the warm solve at full size
                work_alpha = eng.trimap_matte(bgr, tri, *cf)[0]
                bgr = eng.to_device(np.stack([f for _, _, _, f in chunk]))
                alpha, rgba, iters, rel = eng.closed_form_full(bgr, tri, work_alpha, bgr, cf[0], cf[1], args.cf_grow,
                                                               args.cf_full_iters, cf[3])
            if args.decontaminate:
                rgba = eng.estimate_foreground(bgr, alpha, *ForegroundColours().args(), want_rgba=True)[1]
            alpha, rgba, iters, rel = alpha.cpu().numpy(), rgba.cpu().numpy(), iters.cpu().numpy(), rel.cpu().numpy()
            elapsed = (time.perf_counter() - t0) / len(chunk)
            for j, (path, _, trimap, _) in enumerate(chunk):
                n_done += 1
                total_t += elapsed
                stem = out_dir / path.stem
                if "alpha" in args.save:
                    _write_png(f"{stem}_alpha.png", alpha_to_u8(alpha[j]))
                if "cutout" in args.save:
                    rgba[j][..., 3] = alpha_to_u8(alpha[j])       # the byte of the float32 matte: both files agree
                    _write_png(f"{stem}_cutout.png", rgba[j])
                unknown = ((trimap != 0) & (trimap != 255)).mean()
                print(f"[{n_done}/{n_all}] {path.name}  unknown={unknown:.1%}  iterations={int(iters[j])}  "
                      f"residual={float(rel[j]):.2e}  total={elapsed:.4f}s")
    print(f"\n{TAG} {n_done} image(s) → {out_dir}/  ({total_t / n_done:.4f}s per image)")


if __name__ == "__main__":
    sys.exit(main())
