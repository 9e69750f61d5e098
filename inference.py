"""
inference.py — automatic segmentation with GCN-GrabCut on MI355X.

Same command line as the reference's inference.py (flags :26-56, outputs :146-155):

    python3 inference.py --image path/to/image.jpg
    python3 inference.py --input path/to/folder --output results/
    python3 inference.py --image cat.jpg --keep-largest --save mask overlay
    python3 inference.py --image cat.jpg --fg-point 120,200 --bg-point 10,10 --hint-radius 8
    python3 inference.py --image cat.jpg --bg-stroke "40,10 40,200 90,260" --stroke-radius 4   # a brush stroke of three vertices
    python3 inference.py --image cat.jpg --lasso "20,30 20,300 260,300 260,30"   # everything outside the outline is background
    python3 inference.py --image cat.jpg --scissors "40,60 30,220 200,260 230,80"   # four anchors on the outline, traced into a lasso
    python3 inference.py --image cat.jpg --bg-wand "0,0 0,399" --wand-tolerance 24 --save mask selection   # the backdrop by magic wand
    python3 inference.py --image cat.jpg --save mask alpha cutout          # soft edges: alpha matte and cut-out
    python3 inference.py --image big.jpg --full-res --save mask cutout     # outputs at the photo's own size
    python3 inference.py --image big.jpg --full-res --full-mask cut --save mask   # ... the mask cut again on the photo's pixels
    python3 inference.py --image cat.jpg --matte-method closed-form --save alpha cutout   # closed-form matte
    python3 inference.py --image big.jpg --full-res --matte-method closed-form-full --save alpha cutout   # ... solved at the photo's own size
    python3 inference.py --image cat.jpg --background beach.jpg --paste-at 40,120 --composite seamless --save mask composite   # the result on a new background

Images are decoded / written with Pillow (OpenCV is not a dependency of this build); folders are processed in
batches of equally sized images so that the whole batch stays resident in HBM.
"""
import argparse
import json
import time
from pathlib import Path

import numpy as np

IMAGE_EXTS = {".jpg", ".jpeg", ".png", ".bmp", ".tif", ".tiff", ".webp"}


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Automatic GCN-GrabCut segmentation (MI355X)")
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument("--image", help="Path to a single input image")
    src.add_argument("--input", help="Directory of images to segment")
    parser.add_argument("--output", default="results", help="Output directory")
    parser.add_argument("--checkpoint", default="checkpoints/best_model.pt")
    parser.add_argument("--model", default="resgcn", choices=["resgcn", "gcn", "gat"])
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--threshold", type=float, default=0.55, help="Softmax threshold for definite FG/BG superpixels")
    parser.add_argument("--max-size", type=int, default=800, help="Resize longest edge to this before segmenting (0 = off)")
    parser.add_argument("--refine", type=int, default=0, help="Extra GrabCut refinement iterations")
    parser.add_argument("--superpixels", type=int, default=300)
    parser.add_argument("--hidden", type=int, default=128)
    parser.add_argument("--layers", type=int, default=6)
    parser.add_argument("--no-edge-aware", action="store_true",
                        help="Threshold region probabilities directly instead of projecting them through a guided filter")
    parser.add_argument("--filter-radius", type=int, default=8, help="Guided-filter radius for the edge-aware trimap")
    parser.add_argument("--min-area", type=float, default=0.002,
                        help="Drop mask components smaller than this fraction of the image")
    parser.add_argument("--keep-largest", action="store_true", help="Keep only the largest connected component")
    parser.add_argument("--save", nargs="+", default=["mask", "overlay"],
                        choices=["mask", "overlay", "rgba", "trimap", "alpha", "cutout", "outlines", "modified", "selection",
                                 "composite"],
                        help="Which outputs to write (alpha / cutout: the soft matte and the BGRA cut-out with it; "
                             "selection: what the --fg-wand / --bg-wand seeds select, as <prefix>_selection.png; composite: the result "
                             "on --background, as <prefix>_composite.png)")
    # additive: the mask's exact vector outlines (ggc_mask_outlines), written as <prefix>_outlines.json by --save outlines
    parser.add_argument("--outline-connectivity", type=int, choices=[4, 8], default=8,
                        help="--save outlines: 8 joins diagonal foreground pixels into one loop (as the mask clean-up "
                             "labels components), 4 separates them")
    # additive: modify the selection by a distance (ggc_modify_mask), written as <prefix>_modified.png by --save modified
    parser.add_argument("--modify", action="append", type=_modify_step, default=[], metavar="OP:R[:R2]",
                        help="--save modified: grow, shrink, open or close the mask by R pixels, or take its border or a "
                             "trimap with R pixels into the foreground and R2 (default R) into the background, by exact "
                             "Euclidean distance (repeatable, applied in order)")
    parser.add_argument("--batch", type=int, default=64, help="Images per device batch (additive flag)")
    # additive: user clicks as hard constraints (ggc_apply_hints), single-image runs only
    parser.add_argument("--fg-point", action="append", type=_point, default=[], metavar="ROW,COL",
                        help="Foreground click in original-image pixels (repeatable; needs --image)")
    parser.add_argument("--bg-point", action="append", type=_point, default=[], metavar="ROW,COL",
                        help="Background click in original-image pixels (repeatable; needs --image)")
    parser.add_argument("--hint-radius", type=int, default=5,
                        help="Radius in pixels of the image as segmented (after --max-size) painted around each click")
    # additive: geodesic click hints (ggc_geodesic_hints) instead of disks
    parser.add_argument("--hint-mode", choices=["disk", "geodesic"], default="disk",
                        help="How a click is painted: a disk of --hint-radius, or the pixels within a geodesic distance of "
                             "it that does not cross colour edges (--geodesic-radius, --hint-gamma; --hint-radius is ignored)")
    parser.add_argument("--hint-gamma", type=int, default=2, help="Weight of the colour term of the geodesic distance, 0..64")
    parser.add_argument("--geodesic-radius", type=int, default=40,
                        help="Reach of a geodesic click over flat colour, in pixels of the image as segmented, 0..16384")
    # additive: brush strokes as hard constraints (ggc_apply_strokes), single-image runs only
    parser.add_argument("--fg-stroke", action="append", type=_stroke, default=[], metavar='"ROW,COL ROW,COL ..."',
                        help="Foreground brush stroke, a polyline of vertices in original-image pixels (repeatable; needs --image)")
    parser.add_argument("--bg-stroke", action="append", type=_stroke, default=[], metavar='"ROW,COL ROW,COL ..."',
                        help="Background brush stroke, a polyline of vertices in original-image pixels (repeatable; needs --image)")
    parser.add_argument("--stroke-radius", type=int, default=3,
                        help="Brush radius in pixels of the image as segmented (after --max-size), 0..16384; 0 paints the "
                             "centre line; ignored with --hint-mode geodesic, where the centre line is the source set")
    # additive: lassos and filled polygons as hard constraints (ggc_apply_polygons), single-image runs only
    parser.add_argument("--lasso", type=_polygon, default=None, metavar='"ROW,COL ROW,COL ..."',
                        help="Lasso, a closed outline of at least 3 vertices in original-image pixels: everything outside "
                             "it becomes definite background (needs --image)")
    parser.add_argument("--fg-polygon", action="append", type=_polygon, default=[], metavar='"ROW,COL ROW,COL ..."',
                        help="Filled foreground polygon of at least 3 vertices in original-image pixels (repeatable; needs --image)")
    parser.add_argument("--bg-polygon", action="append", type=_polygon, default=[], metavar='"ROW,COL ROW,COL ..."',
                        help="Filled background polygon of at least 3 vertices in original-image pixels (repeatable; needs --image)")
    # additive: the magic wand (ggc_wand_select): seeds select the pixels that look like them, single-image runs only
    parser.add_argument("--fg-wand", action="append", type=_stroke, default=[], metavar='"ROW,COL ROW,COL ..."',
                        help="Foreground magic-wand seeds in original-image pixels: what each selects becomes definite "
                             "foreground (repeatable; needs --image)")
    parser.add_argument("--bg-wand", action="append", type=_stroke, default=[], metavar='"ROW,COL ROW,COL ..."',
                        help="Background magic-wand seeds in original-image pixels: what each selects becomes definite "
                             "background, over the foreground seeds' (repeatable; needs --image)")
    parser.add_argument("--wand-tolerance", type=int, default=32,
                        help="How far a pixel's colour may lie from a seed's, 0..255, in the channel that differs most")
    parser.add_argument("--wand-connectivity", type=int, choices=[4, 8, 0], default=8,
                        help="Neighbours through which a selection spreads from its seed; 0 selects every similar pixel, "
                             "connected to the seed or not")
    parser.add_argument("--wand-sample", type=int, choices=[1, 3, 5], default=1,
                        help="Side of the window around a seed whose mean colour is the seed's colour")
    # additive: intelligent scissors (ggc_trace_paths): a few anchors on the outline, traced into a lasso
    parser.add_argument("--scissors", action="append", type=_polygon, default=[], metavar='"ROW,COL ROW,COL ..."',
                        help="Anchors on the object's outline, at least 3, in order and in original-image pixels: they are "
                             "joined along the image's edges into a closed outline that acts as a lasso (repeatable; "
                             "needs --image)")
    parser.add_argument("--scissors-margin", type=int, default=16,
                        help="Pixels, 0..256, that a traced segment may leave the bounding box of its two anchors")
    parser.add_argument("--scissors-edge-cap", type=int, default=2048,
                        help="Gradient, 1..13770, at which an edge counts as fully strong")
    parser.add_argument("--scissors-smooth", type=int, default=16,
                        help="Cost per step, 1..64, that does not depend on the image: larger keeps the outline shorter")
    # additive: soft alpha matte of the mask (ggc_alpha_matte), computed when --save asks for alpha or cutout
    parser.add_argument("--matte-radius", type=int, default=4,
                        help="Window radius of the alpha matte, 1..64, in pixels of the image as segmented")
    parser.add_argument("--matte-eps", type=float, default=1e-4, help="Regularisation of the alpha matte (>= 1e-12)")
    # additive: the closed-form matte (ggc_closed_form_matte) instead of the guided one; its own window and regulariser
    parser.add_argument("--matte-method", choices=["guided", "closed-form", "closed-form-full"], default="guided",
                        help="How alpha / cutout are computed: guided-filter feathering of the mask (--matte-radius, "
                             "--matte-eps), the closed-form matte solved on a band around its edge (--cf-* flags), or "
                             "that matte solved again at the original size from the working-size one (closed-form-full: "
                             "needs --full-res; --cf-grow, --cf-full-iters)")
    parser.add_argument("--cf-radius", type=int, default=1, help="Window radius of the closed-form matte, 1..8")
    parser.add_argument("--cf-eps", type=float, default=1e-5, help="Regularisation of the closed-form matte, [1e-12, 1]")
    parser.add_argument("--cf-band", type=int, default=1,
                        help="Half-width in pixels of the unknown band around the mask's edge, 0..64")
    parser.add_argument("--cf-iters", type=int, default=500, help="Most conjugate-gradient iterations per image")
    parser.add_argument("--cf-tol", type=float, default=1e-4, help="Stop when the residual falls to this fraction")
    parser.add_argument("--cf-grow", type=int, default=0,
                        help="closed-form-full: pixels of the original size the lifted unknown band is grown by, 0..64")
    parser.add_argument("--cf-full-iters", type=int, default=2000,
                        help="closed-form-full: most conjugate-gradient iterations per image at the original size")
    # additive: foreground colours under the matte (ggc_estimate_foreground), so that the cut-out carries no old background
    parser.add_argument("--decontaminate", action="store_true",
                        help="Write the cut-out (--save cutout) with estimated foreground colours where alpha is "
                             "fractional, instead of the image's own, so that it shows no halo on a new background")
    parser.add_argument("--decon-eps", type=float, default=5e-3, help="Constant part of the colour smoothness weight, [0, 1]")
    parser.add_argument("--decon-omega", type=float, default=1.0,
                        help="Weight of |alpha_i - alpha_j| in the colour smoothness weight, [0, 1000]")
    parser.add_argument("--decon-iters", type=int, default=2000, help="Most conjugate-gradient iterations per image")
    parser.add_argument("--decon-tol", type=float, default=1e-6, help="Stop when the residual falls to this fraction")
    # additive: outputs at the original size (ggc_upsample_matte), for images that --max-size shrank
    parser.add_argument("--full-res", action="store_true",
                        help="Write every output at the original image size: the mask (and alpha) found at --max-size "
                             "is carried to the original by a fast guided filter with --matte-radius / --matte-eps, the "
                             "trimap by nearest neighbour; images already within --max-size are unaffected")
    # additive: the hard mask at the original size by a banded graph cut there (ggc_lift_labels, ggc_grabcut)
    parser.add_argument("--full-mask", choices=["guided", "cut"], default="guided",
                        help="With --full-res, how the hard mask (mask, overlay, rgba) reaches the original size: the "
                             "guided upsample's alpha >= 0.5, or GrabCut run again on the original pixels inside a band "
                             "around the lifted mask's edge (cut: --full-cut-band, --full-cut-iters)")
    parser.add_argument("--full-cut-band", type=int, default=None,
                        help="--full-mask cut: half-width of the open band in original pixels, 0..64 "
                             "(default: one and a half working pixels)")
    parser.add_argument("--full-cut-iters", type=int, default=1, help="--full-mask cut: GrabCut iterations at the original size")
    # additive: the result placed on another picture (ggc_composite_over, ggc_poisson_clone), written by --save composite
    parser.add_argument("--background", default=None,
                        help="--save composite: the picture every result is placed on")
    parser.add_argument("--paste-at", type=_point, default=(0, 0), metavar="ROW,COL",
                        help="Row and column of --background where the result's top-left pixel lands (may be negative: --paste-at=-3,12)")
    parser.add_argument("--composite", choices=["over", "seamless", "mixed"], default="over",
                        help="How the result is placed: alpha-over of its cleanest cut-out, or the image under its mask "
                             "cloned in the gradient domain with the image's (seamless) or with mixed gradients")
    return parser


def _point(text: str):
    try:
        r, c = (int(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected ROW,COL (two integers), got '{text}'")
    return r, c


def _stroke(text: str):
    try:
        pts = [_point(v) for v in text.split()]
    except argparse.ArgumentTypeError:
        pts = []
    if not pts:
        raise argparse.ArgumentTypeError(f"expected 'ROW,COL ROW,COL ...' (at least one vertex), got '{text}'")
    return pts


def _polygon(text: str):
    try:
        pts = [_point(v) for v in text.split()]
    except argparse.ArgumentTypeError:
        pts = []
    if len(pts) < 3:
        raise argparse.ArgumentTypeError(f"expected 'ROW,COL ROW,COL ROW,COL ...' (at least three vertices), got '{text}'")
    return pts


def _modify_step(text: str):
    """OP:R[:R2] -> a ModifyMask step."""
    from src.gcn_grabcut import ModifyMask
    parts = text.split(":")
    try:
        if len(parts) not in (2, 3):
            raise ValueError("expected OP:R or OP:R:R2")
        return ModifyMask(parts[0], float(parts[1]), float(parts[2]) if len(parts) == 3 else None)
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"--modify {text!r}: {e}")


def wand_options(parser, args):
    """The Wand of --wand-* when the run has wand seeds, else None; parser.error on options that do not fit together."""
    seeds = bool(args.fg_wand or args.bg_wand)
    if seeds and not args.image:
        parser.error("--fg-wand / --bg-wand are seeds on one image: use them with --image, not --input")
    if "selection" in args.save and not seeds:
        parser.error("--save selection writes what --fg-wand / --bg-wand seeds select: give at least one")
    if not seeds:
        return None
    from src.gcn_grabcut import Wand
    try:
        return Wand(args.wand_tolerance, args.wand_connectivity or 8, args.wand_connectivity != 0, args.wand_sample)
    except ValueError as e:
        parser.error(str(e))


def outlines_document(shape, outlines, connectivity: int) -> dict:
    """What --save outlines writes: the loops of a mask of `shape` on its corner lattice, (row, col) vertices with area,
    perimeter and outer loop each, and all of them as one SVG path (x = col, y = row) for fill-rule="evenodd"."""
    from src.gcn_grabcut import outlines_svg_path
    return {"height": int(shape[0]), "width": int(shape[1]), "connectivity": int(connectivity),
            "loops": [{"vertices": [[int(r), int(c)] for r, c in o.vertices], "area": int(o.area),
                       "perimeter": int(o.perimeter), "outer": int(o.outer)} for o in outlines],
            "svg_path": outlines_svg_path(outlines)}


def scale_points(points, orig_hw, new_hw):
    """Clicks given in the original image -> the pixels they fall on after read_bgr's resize."""
    (h0, w0), (h1, w1) = orig_hw, new_hw
    return [(r * h1 // h0, c * w1 // w0) for r, c in points]


def read_bgr(path: Path, max_size: int, keep_original: bool = False):
    """The image as BGR uint8, its longest side shrunk to max_size; keep_original=True -> (that, the decoded original)."""
    from PIL import Image
    try:
        im = Image.open(path).convert("RGB")
    except Exception:
        return None
    orig = im
    if max_size > 0:
        w, h = im.size
        scale = min(max_size / max(h, w), 1.0)
        if scale < 1.0:
            im = im.resize((int(w * scale), int(h * scale)), Image.BOX)   # area averaging, as cv2.INTER_AREA
    bgr = np.ascontiguousarray(np.asarray(im)[:, :, ::-1])
    if keep_original:
        return bgr, (bgr if orig is im else np.ascontiguousarray(np.asarray(orig)[:, :, ::-1]))
    return bgr


def load_model(checkpoint: str, model_name: str = "resgcn", hidden: int = 128, layers: int = 6, device: str = "cuda",
               tag: str = "inference"):
    """The trimap network of a train.py checkpoint, in eval mode; its width and depth come from the checkpoint."""
    import torch
    from src.gcn_grabcut.model import GATTrimapNet, GCNTrimapNet, ResGCNNet

    if not torch.cuda.is_available():
        raise SystemExit(f"[{tag}] no MI355X visible: this build has no CPU path")
    model_cls = {"resgcn": ResGCNNet, "gcn": GCNTrimapNet, "gat": GATTrimapNet}[model_name]

    ckpt_path = Path(checkpoint)
    if not ckpt_path.exists():
        fallback = Path("checkpoints/final_model.pt")
        if not fallback.exists():
            raise FileNotFoundError(f"No checkpoint at {ckpt_path} (or {fallback}). Train one with train.py.")
        print(f"[{tag}] {ckpt_path} not found, using {fallback}")
        ckpt_path = fallback
    state = torch.load(ckpt_path, map_location="cpu", weights_only=True)["model"]
    # width and depth are recovered from the checkpoint (reference inference.py:81-86)
    hidden = state["input_proj.0.weight"].shape[0] if "input_proj.0.weight" in state else hidden
    layers = (sum(1 for k in state if k.startswith("gcn_layers.") and k.endswith(".bias"))
              or sum(1 for k in state if k.startswith("blocks.") and k.endswith(".conv.bias"))
              or sum(1 for k in state if k.startswith("convs.") and k.endswith(".att")) or layers)
    model = model_cls(hidden_channels=hidden, n_layers=layers)
    model.load_state_dict(state)
    model.eval()
    print(f"[{tag}] loaded {model_cls.__name__} (D={hidden}, n={layers}) from {ckpt_path} on {device}")
    return model


def main() -> None:
    parser = build_parser()
    args = parser.parse_args()
    if (args.fg_point or args.bg_point) and not args.image:
        parser.error("--fg-point / --bg-point are clicks on one image: use them with --image, not --input")
    if (args.fg_stroke or args.bg_stroke) and not args.image:
        parser.error("--fg-stroke / --bg-stroke are strokes on one image: use them with --image, not --input")
    if (args.lasso or args.fg_polygon or args.bg_polygon) and not args.image:
        parser.error("--lasso / --fg-polygon / --bg-polygon are polygons on one image: use them with --image, not --input")
    scissors_options = None
    if args.scissors:
        if not args.image:
            parser.error("--scissors are anchors on one image: use them with --image, not --input")
        from src.gcn_grabcut import Scissors
        try:
            scissors_options = Scissors(args.scissors_margin, args.scissors_edge_cap, args.scissors_smooth)
        except ValueError as e:
            parser.error(str(e))
    wand = wand_options(parser, args)
    if bool(args.modify) != ("modified" in args.save):
        parser.error("--modify steps are written by --save modified: give both or neither")
    if not 0 <= args.stroke_radius <= 16384:
        parser.error("--stroke-radius must be in 0..16384")
    if args.hint_radius < 0:
        parser.error("--hint-radius must be >= 0")
    if not 0 <= args.hint_gamma <= 64:
        parser.error("--hint-gamma must be in 0..64")
    if not 0 <= args.geodesic_radius <= 16384:
        parser.error("--geodesic-radius must be in 0..16384")
    matte = "alpha" in args.save or "cutout" in args.save
    if (matte or args.full_res) and not 1 <= args.matte_radius <= 64:
        parser.error("--matte-radius must be in 1..64")
    if (matte or args.full_res) and not args.matte_eps >= 1e-12:
        parser.error("--matte-eps must be >= 1e-12")
    closed_form = None
    if args.matte_method == "closed-form-full" and not args.full_res:
        parser.error("--matte-method closed-form-full solves at the original size: add --full-res")
    if matte and args.matte_method in ("closed-form", "closed-form-full"):
        full_solve = args.matte_method == "closed-form-full"
        if args.full_res and not full_solve:
            parser.error("--matte-method closed-form is not carried to the original size: drop --full-res, use "
                         "--matte-method guided, or solve there with --matte-method closed-form-full")
        from src.gcn_grabcut.pipeline import ClosedFormMatte, _closed_form_full_args
        from src.gcn_grabcut._engine import check_closed_form_args
        closed_form = ClosedFormMatte(args.cf_radius, args.cf_eps, args.cf_band, args.cf_iters, args.cf_tol,
                                      full_resolution=full_solve, grow=args.cf_grow, full_max_iter=args.cf_full_iters)
        try:
            check_closed_form_args(*closed_form.args())
            _closed_form_full_args(closed_form)
        except ValueError as e:
            parser.error(str(e))
    full_cut = None
    if args.full_mask == "cut":
        if not args.full_res:
            parser.error("--full-mask cut cuts at the original size: add --full-res")
        if args.matte_method == "closed-form-full":
            parser.error("--full-mask cut cannot be combined with --matte-method closed-form-full, whose mask is its "
                         "alpha >= 0.5: use --matte-method guided")
        from src.gcn_grabcut.pipeline import FullCut, _full_cut_args
        full_cut = FullCut(args.full_cut_band, args.full_cut_iters)
        try:
            _full_cut_args(full_cut, True, None)
        except ValueError as e:
            parser.error(str(e))
    foreground = None
    if args.decontaminate:
        if "cutout" not in args.save:
            parser.error("--decontaminate changes the cut-out: add cutout to --save")
        if args.full_res:
            parser.error("--decontaminate is not carried to the original size: drop --full-res")
        from src.gcn_grabcut.pipeline import ForegroundColours
        from src.gcn_grabcut._engine import check_foreground_args
        foreground = ForegroundColours(args.decon_eps, args.decon_omega, args.decon_iters, args.decon_tol)
        try:
            check_foreground_args(*foreground.args())
        except ValueError as e:
            parser.error(str(e))
    background = None
    if (args.background is not None) != ("composite" in args.save):
        parser.error("--background is what --save composite places the result on: give both or neither")
    if args.background is not None:
        if max(abs(v) for v in args.paste_at) > 32768:
            parser.error("--paste-at must lie within +-32768")
        background = read_bgr(Path(args.background), 0)
        if background is None:
            parser.error(f"cannot read --background {args.background}")
    from src.gcn_grabcut import GCNGrabCutPipeline
    from src.gcn_grabcut.graph_builder import SuperpixelGraphConfig
    from src.gcn_grabcut.pipeline import _colour_trimap, _write_png, alpha_to_u8, nearest_upsample

    model = load_model(args.checkpoint, args.model, args.hidden, args.layers, args.device)

    pipeline = GCNGrabCutPipeline(model, sp_config=SuperpixelGraphConfig(n_segments=args.superpixels), device=args.device)

    if args.image:
        paths = [Path(args.image)]
    else:
        in_dir = Path(args.input)
        paths = sorted(p for p in in_dir.iterdir() if p.suffix.lower() in IMAGE_EXTS)
        if not paths:
            raise FileNotFoundError(f"No images found in {in_dir}")
    out_dir = Path(args.output)
    out_dir.mkdir(parents=True, exist_ok=True)

    by_shape: dict = {}
    for path in paths:
        image = read_bgr(path, args.max_size, keep_original=args.full_res)
        if image is None:
            print(f"[inference] skipping unreadable file: {path}")
            continue
        if args.full_res:                               # grouped by (working shape, original shape)
            image, orig = image
            full = orig if orig.shape != image.shape else None
            by_shape.setdefault((image.shape, orig.shape), []).append((path, image, full))
        else:
            by_shape.setdefault(image.shape, []).append((path, image, None))

    total_t, n_done = 0.0, 0
    for items in by_shape.values():
        for i in range(0, len(items), args.batch):
            chunk = items[i:i + args.batch]
            t0 = time.perf_counter()
            hint_kw = {}
            polygons = args.lasso or args.fg_polygon or args.bg_polygon
            if args.fg_point or args.bg_point or args.fg_stroke or args.bg_stroke or polygons or args.scissors or wand:   # --image only: one chunk of one image
                from PIL import Image
                path, image, _ = chunk[0]
                with Image.open(path) as im:
                    orig_hw = im.size[::-1]
                if args.fg_point or args.bg_point:
                    hint_kw = dict(hints=[(scale_points(args.fg_point, orig_hw, image.shape[:2]),
                                           scale_points(args.bg_point, orig_hw, image.shape[:2]))],
                                   hint_radius=args.hint_radius)
                if args.fg_stroke or args.bg_stroke:
                    hint_kw.update(strokes=[([scale_points(s, orig_hw, image.shape[:2]) for s in args.fg_stroke],
                                             [scale_points(s, orig_hw, image.shape[:2]) for s in args.bg_stroke])],
                                   stroke_radius=args.stroke_radius)
                if polygons:
                    hint_kw.update(polygons=[([scale_points(p, orig_hw, image.shape[:2]) for p in args.fg_polygon],
                                              [scale_points(p, orig_hw, image.shape[:2]) for p in args.bg_polygon],
                                              [scale_points(args.lasso, orig_hw, image.shape[:2])] if args.lasso else [])])
                if args.scissors:
                    hint_kw.update(scissors=[[scale_points(a, orig_hw, image.shape[:2]) for a in args.scissors]],
                                   scissors_options=scissors_options)
                if wand is not None:
                    wand_seeds = (scale_points([p for s in args.fg_wand for p in s], orig_hw, image.shape[:2]),
                                  scale_points([p for s in args.bg_wand for p in s], orig_hw, image.shape[:2]))
                    hint_kw.update(wands=[wand_seeds], wand=wand)
                if args.hint_mode == "geodesic":
                    from src.gcn_grabcut import GeodesicHints
                    hint_kw.update(geodesic=GeodesicHints(args.geodesic_radius, args.hint_gamma))
            if closed_form is not None:                 # an image within --max-size is already solved at its own size
                import dataclasses
                hint_kw.update(matte=closed_form if chunk[0][2] is not None else
                               dataclasses.replace(closed_form, full_resolution=False))
            elif matte:
                hint_kw.update(matte=True, matte_radius=args.matte_radius, matte_eps=args.matte_eps)
            if foreground is not None:
                hint_kw.update(foreground=foreground)
            if chunk[0][2] is not None:                 # --full-res on images that --max-size shrank
                hint_kw.update(full_images=[full for _, _, full in chunk], matte_radius=args.matte_radius,
                               matte_eps=args.matte_eps)
                if full_cut is not None:
                    hint_kw.update(full_cut=full_cut)
            results = pipeline.segment_batch(
                [im for _, im, _ in chunk], threshold_fg=args.threshold, threshold_bg=args.threshold,
                refine_iters=args.refine, min_area_ratio=args.min_area, keep_largest=args.keep_largest,
                edge_aware=not args.no_edge_aware, filter_radius=args.filter_radius, **hint_kw)
            elapsed = (time.perf_counter() - t0) / len(chunk)
            for (path, _, _), result in zip(chunk, results):
                total_t += elapsed
                n_done += 1
                stem = out_dir / path.stem
                out = result if result.full is None else result.full          # every file at one size
                if "mask" in args.save:
                    _write_png(f"{stem}_mask.png", out.binary_mask * 255)
                if "overlay" in args.save:
                    _write_png(f"{stem}_overlay.png", out.overlay)
                if "rgba" in args.save:
                    _write_png(f"{stem}_rgba.png", out.rgba)
                if "trimap" in args.save:
                    trimap = result.trimap if result.full is None else nearest_upsample(result.trimap,
                                                                                        *out.binary_mask.shape)
                    _write_png(f"{stem}_trimap.png", _colour_trimap(trimap))
                if "alpha" in args.save:
                    _write_png(f"{stem}_alpha.png", alpha_to_u8(out.alpha))
                if "cutout" in args.save:
                    _write_png(f"{stem}_cutout.png", out.rgba_soft if foreground is None else result.rgba_clean)
                if "outlines" in args.save:                 # on the grid of the mask file written above
                    loops = result.outlines(args.outline_connectivity, full=result.full is not None)
                    with open(f"{stem}_outlines.json", "w") as f:
                        json.dump(outlines_document(out.binary_mask.shape, loops, args.outline_connectivity), f)
                if "selection" in args.save:                # the wand's own selection, at the size the image was segmented at
                    from src.gcn_grabcut import wand_select
                    _write_png(f"{stem}_selection.png", wand_select(result.image, *wand_seeds, wand, device=args.device))
                if "modified" in args.save:                 # the mask file written above after the --modify steps
                    modified = result.modified(*args.modify, full=result.full is not None)
                    _write_png(f"{stem}_modified.png", modified if modified.max(initial=0) > 1 else modified * 255)
                if "composite" in args.save:                # the files written above, placed on --background
                    _write_png(f"{stem}_composite.png", result.composite_onto(background, args.paste_at, args.composite,
                                                                              full=result.full is not None))
                t = result.timing
                print(f"[{n_done}/{len(paths)}] {path.name}  fg={result.binary_mask.mean():.1%}  "
                      f"graph={t.get('graph_build', 0):.4f}s gcn={t.get('gcn_inference', 0):.4f}s "
                      f"grabcut={t.get('grabcut', 0):.4f}s  total={elapsed:.4f}s")
    if n_done:
        print(f"\n[inference] {n_done} image(s) → {out_dir}/  ({total_t / n_done:.4f}s per image)")
    else:
        print("[inference] nothing to do.")


if __name__ == "__main__":
    main()
