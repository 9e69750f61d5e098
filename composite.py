"""
composite.py — a cut-out placed on a new background on MI355X.  No segmentation is run.

    python3 composite.py --cutout cat_cutout.png --background beach.jpg --at 40,120 --save out.png
    python3 composite.py --image cat.jpg --mask cat_mask.png --background beach.jpg --method seamless --at 40,120 --save out.png
    python3 composite.py --image cat.jpg --mask cat_mask.png --background beach.jpg --method mixed --save out.png

--cutout is a PNG with an alpha channel (inference.py's or matte.py's <stem>_cutout.png): it is placed by alpha-over,
in integer arithmetic (gcn_grabcut.composite_over, ggc_composite_over).  --image with --mask (any nonzero byte selected,
for instance inference.py's <stem>_mask.png) is cloned in the gradient domain, the "seamless" paste of image editors
(gcn_grabcut.seamless_clone, ggc_poisson_clone): --method seamless keeps the image's gradients inside
the mask, --method mixed the stronger of the image's and the background's.  --at R,C is the row and column of the
background at which the cut-out's (or the image's) top-left pixel lands; it may be negative (written --at=-3,12, so
that the value is not read as a flag).
"""
import argparse
import sys
from pathlib import Path

import numpy as np

TAG = "[composite]"


def parse_at(text: str) -> "tuple[int, int]":
    """R,C -> (row, col)."""
    parts = text.split(",")
    try:
        if len(parts) != 2:
            raise ValueError
        return int(parts[0]), int(parts[1])
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected R,C (two integers), got {text!r}")


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Place a cut-out on a new background (MI355X)")
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument("--cutout", help="A BGRA cut-out (PNG with alpha): placed by alpha-over")
    src.add_argument("--image", help="An image (with --mask): cloned in the gradient domain")
    parser.add_argument("--mask", default=None, help="Mask of --image: any nonzero byte selected")
    parser.add_argument("--background", required=True, help="The picture the cut-out is placed on")
    parser.add_argument("--at", type=parse_at, default=(0, 0), metavar="R,C",
                        help="Row and column of the background where the source's top-left pixel lands (may be negative: --at=-3,12)")
    parser.add_argument("--method", default=None, choices=["over", "seamless", "mixed"],
                        help="over (with --cutout, the default there) | seamless | mixed (with --image and --mask)")
    parser.add_argument("--save", default="composite.png", help="Output file")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--clone-iters", type=int, default=None, help="Most conjugate-gradient iterations of a clone")
    parser.add_argument("--clone-tol", type=float, default=None, help="Stop a clone when the residual falls to this fraction")
    return parser


def check_args(parser: argparse.ArgumentParser, args) -> None:
    """The rules between the flags; parser.error on a bad combination."""
    if args.cutout:
        if args.mask is not None:
            parser.error("--mask goes with --image, not --cutout")
        if args.method not in (None, "over"):
            parser.error("--cutout is placed by alpha-over: --method seamless and mixed take --image and --mask")
        args.method = "over"
    else:
        if args.mask is None:
            parser.error("--image goes with --mask")
        if args.method == "over":
            parser.error("--method over takes --cutout; --image and --mask take seamless or mixed")
        args.method = args.method or "seamless"
    if abs(args.at[0]) > 32768 or abs(args.at[1]) > 32768:
        parser.error("--at must lie within +-32768")


def _read(path: str, mode: str) -> np.ndarray:
    from PIL import Image
    try:
        with Image.open(path) as im:
            a = np.asarray(im.convert(mode), dtype=np.uint8)
    except Exception:
        raise SystemExit(f"{TAG} cannot read {path}")
    if mode == "RGB":
        a = a[:, :, ::-1]
    elif mode == "RGBA":
        a = a[:, :, [2, 1, 0, 3]]
    return np.ascontiguousarray(a)


def main(argv=None) -> None:
    parser = build_parser()
    args = parser.parse_args(argv)
    check_args(parser, args)
    from src.gcn_grabcut.pipeline import CLONE_MAX_ITER, CLONE_TOL, Clone, _write_png, composite_over, seamless_clone
    clone = None
    if args.method != "over":
        try:
            clone = Clone(args.method == "mixed", CLONE_MAX_ITER if args.clone_iters is None else args.clone_iters,
                          CLONE_TOL if args.clone_tol is None else args.clone_tol)
        except ValueError as e:
            parser.error(str(e))
    background = _read(args.background, "RGB")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{TAG} no MI355X visible: this build has no CPU path")
    try:
        if args.method == "over":
            out = composite_over(_read(args.cutout, "RGBA"), background, args.at, device=args.device)
            note = "alpha-over"
        else:
            image, mask = _read(args.image, "RGB"), _read(args.mask, "L")
            if mask.shape != image.shape[:2]:
                raise SystemExit(f"{TAG} {args.mask} is {mask.shape[1]}x{mask.shape[0]} but {args.image} is "
                                 f"{image.shape[1]}x{image.shape[0]}")
            out, n, iters, rel = seamless_clone(image, mask, background, args.at, *clone.args(), return_info=True,
                                                device=args.device)
            note = f"{args.method} clone of {n} pixels, iterations={iters} residual={rel:.2e}"
    except ValueError as e:
        raise SystemExit(f"{TAG} {e}")
    Path(args.save).parent.mkdir(parents=True, exist_ok=True)
    _write_png(args.save, out)
    print(f"{TAG} {note} → {args.save}")


if __name__ == "__main__":
    sys.exit(main())
