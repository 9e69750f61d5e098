"""Feature fuzzer (a checker, hence under tests/; the sibling of tests/fuzz_parity.py): random shapes, batches and primitives
through the interactive and post entries, every output array_equal to the integer restatement of include/ggc.h that the
entry's own test file already holds.  Families: clicks (ggc_apply_hints), geodesic (ggc_geodesic_hints), strokes
(ggc_apply_strokes), stroke_pixels (ggc_stroke_pixels, its rows then through ggc_apply_hints), polygons
(ggc_apply_polygons), scissors (ggc_trace_paths, its vertices then through ggc_apply_polygons as lassos), next_click
(ggc_next_click), clean (ggc_clean_mask), eval_counts (ggc_eval_counts) and matte (ggc_matte_errors); and, because they
share a scratch slot with one of those (S_CC_C with clean-up, S_MISC_A with clicks) and zero it themselves, mask_iou
(ggc_mask_iou, against numpy counts) and seed_prior (ggc_seed_from_prior, against the oracle).

Three layers.  The generators are pure numpy: case i of a family is a function of (family, seed, i) alone (its generator is
child i of SeedSequence((family id, seed))).  The references are the restatements, on the CPU.  The device runners import
the engine inside their functions, so the first two layers import and run without a GPU (tests/test_fuzz_features_cpu.py);
tests/test_fuzz_features_gpu.py runs 40 cases per family at two seeds, and all of them interleaved on one context.

Shapes walk EDGES, the tile and wave boundaries of csrc/ggc_paint.h (32x8), ggc_relax.h (32x32) and ggc_ccl.h (64 lanes)
+-1: the first len(EDGES) cases take them as H, the next as W, the rest draw both sides (from EDGES with probability 0.6,
else 3..110).  Case 0 is 1x1.  The cheap families (next_click, clean, eval_counts) also walk 255..257.

    python tests/fuzz_features.py --family strokes --seed 7 --case 12     one case: its mismatch line(s), or ok
    FUZZ_N=400 FUZZ_SEED=11 python tests/fuzz_features.py --family clean  a long pass of one family (no --family: of all)

A mismatch is one line: family, seed, case, BxHxW, the drawn parameters, the output that differs, in how many elements,
and the first differing index.

Not testable: "a sentinel stays in every geodesic output not asked for".  Where ggc_geodesic_hints is asked for a subset of
its four outputs the others are passed as NULL, so there is no array of theirs that could hold a sentinel.  (Half of the
geodesic masks are filled with 7, a value no entry writes; that checks the pixels the rule does not paint, as for strokes
and polygons, and says nothing about outputs not asked for.)

Long pass 1 (by hand, one process per family, seed 11, FUZZ_N=400; the suite's seeds are 1 and 2):
clicks 400 cases, 0 mismatches, <1 s; geodesic 400, 0, 17 s; strokes 400, 0, 6 s; stroke_pixels 400, 0, 12 s; polygons
400, 0, 1 s; scissors 400, 0, 13 s; next_click 400, 0, 1 s; clean 400, 0, 1 s; eval_counts 400, 0, <1 s; matte 400, 0,
1 s; mask_iou 400, 0, <1 s; seed_prior 400, 0, <1 s (wall time of references and device calls together): no mismatch,
4800 cases.  Against a library with four in-bounds mutations
(relax_box's upper row bound at RX_H - 2; paint_slot handing out its slots in reverse order; k_click_pick's tie as >=;
ccl_best_key preferring the larger root) the suite's pass fails in clicks, strokes, stroke_pixels, polygons (paint),
geodesic, scissors (relax), next_click and clean, and passes in eval_counts and matte, which the mutations do not reach."""
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))          # the repository this script sits in
for _p in (os.path.join(R, "tests"), os.path.join(R, "src"), R):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np

import geodesic_ref
import matte_eval_ref
import polygons_ref
import scissors_ref
import strokes_ref
import test_clean_mask_small_gpu as clean_tests
import test_geodesic_gpu as geodesic_tests
import test_hints_gpu as hints_tests
import test_matte_eval_gpu as matte_tests
import test_next_click_gpu as click_tests
import test_polygons_gpu as polygon_tests
import test_scissors_gpu as scissors_tests
import test_strokes_gpu as stroke_tests

EDGES = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 95, 96, 97]
EDGES_CHEAP = EDGES + [255, 256, 257]          # k_click_cols' 256-lane column blocks, the 256-thread raster blocks
FAMILIES = ("clicks", "geodesic", "strokes", "stroke_pixels", "polygons", "scissors", "next_click", "clean", "eval_counts",
            "matte", "mask_iou", "seed_prior")
CHEAP = ("next_click", "clean", "eval_counts")
ORACLE_FAMILIES = ("clean", "eval_counts", "seed_prior")     # their reference is the CPU oracle, handed in by the caller
# stroke_pixels runs on the strokes family's segments, mask_iou on the eval_counts family's masks
SHARES_CASES = {"stroke_pixels": "strokes", "mask_iou": "eval_counts"}
N_CASES = 40
SUITE_SEEDS = (1, 2)
POISON = 7
BATCHES = (1, 2, 3, 5)
IOU_ATOL = 1e-12                               # test_grabcut_gpu.py's bound on ggc_mask_iou's float64 quotient
REFUSED = "the entry returned"                 # marks the line of a case whose entry gave up (run_case)
GAVE_UP = []                                   # those lines, for whoever must not touch the context again


# ---------------------------------------------------------------- layer 1: the generators (numpy only)

def edges_of(family):
    return EDGES_CHEAP if SHARES_CASES.get(family, family) in CHEAP else EDGES


def case_rng(family, seed, index):
    fid = FAMILIES.index(SHARES_CASES.get(family, family))
    return np.random.default_rng(np.random.SeedSequence((fid, int(seed)), spawn_key=(int(index),)))


def _side(rng, edges):
    e, u = int(edges[int(rng.integers(len(edges)))]), int(rng.integers(3, 111))
    return e if rng.random() < 0.6 else u


def draw_shape(rng, index, edges):
    """The schedule: EDGES as H, then as W, then both sides drawn; case 0 is 1x1."""
    a, b = _side(rng, edges), _side(rng, edges)
    n = len(edges)
    if index == 0:
        return 1, 1
    if index < n:
        return edges[index], a
    if index < 2 * n:
        return a, edges[index - n]
    return a, b


def coord(rng, n):
    """Half of the coordinates a multiple of 8 (the tiles are 8, 32 and 64 wide) -1, +0 or +1, the rest uniform in [-4, n+4)."""
    tile = 8 * int(rng.integers(0, (n + 7) // 8 + 1)) + int(rng.integers(-1, 2))
    free = int(rng.integers(-4, n + 4))
    return tile if rng.random() < 0.5 else free


def point(rng, h, w):
    return coord(rng, h), coord(rng, w)


def anchor(rng, h, w):
    r, c = point(rng, h, w)
    return min(max(r, 0), h - 1), min(max(c, 0), w - 1)


def draw_images(rng, b, h, w):
    """(kind, (B,H,W,3) uint8): 0 noise, 1 one flat colour, 2 two flat halves with a darker lower half, 3 the same +-3."""
    kind = int(rng.integers(0, 4))
    noise = rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
    colour = rng.integers(60, 256, 3)
    if kind == 0:
        return kind, noise
    imgs = np.empty((b, h, w, 3), np.int64)
    imgs[:] = colour
    if kind >= 2:
        imgs[:, h // 2:] = colour // 3
    if kind == 3:
        imgs += noise.astype(np.int64) % 7 - 3
    return kind, np.clip(imgs, 0, 255).astype(np.uint8)


def _masks(rng, b, h, w):
    """(poison, masks): GrabCut labels 0..3, or in half of the cases a value no entry writes."""
    labels = rng.integers(0, 4, (b, h, w)).astype(np.uint8)
    poison = bool(rng.random() < 0.5)
    return poison, (np.full((b, h, w), POISON, np.uint8) if poison else labels)


def _segments(rng, b, h, w):
    return np.stack([hints_tests._block_segments(rng, h, w) for _ in range(b)])


def _clicks(rng, b, h, w, empty, most):
    out = []
    for i in range(b):
        n = int(rng.integers(1, most + 1))
        pts = [point(rng, h, w) for _ in range(n)]
        k = int(rng.integers(0, n + 1))
        out.append(None if i == empty else (pts[:k], pts[k:]))
    return out


def gen_clicks(rng, b, h, w, empty):
    radius, region = int(rng.choice([0, 1, 3, 7, 40])), int(rng.integers(0, 2))
    return dict(params=dict(radius=radius, region=region), masks=rng.integers(0, 4, (b, h, w)).astype(np.uint8),
                segs=_segments(rng, b, h, w), per_image=_clicks(rng, b, h, w, empty, 40))


def gen_geodesic(rng, b, h, w, empty):
    gamma, radius = geodesic_tests.SETTINGS[int(rng.integers(len(geodesic_tests.SETTINGS)))]
    kind, imgs = draw_images(rng, b, h, w)
    poison, masks = _masks(rng, b, h, w)
    bits = int(rng.integers(1, 16))
    outputs = tuple(n for i, n in enumerate(("mask", "dist_fg", "dist_bg", "node_dist")) if (bits >> i) & 1)
    return dict(params=dict(gamma=gamma, radius=radius, image_kind=kind, poison=poison, outputs=outputs), imgs=imgs,
                masks=masks, segs=_segments(rng, b, h, w), per_image=_clicks(rng, b, h, w, empty, 12), outputs=outputs)


def gen_strokes(rng, b, h, w, empty):
    radius = int(rng.choice([0, 1, 3, 9, 40]))
    per_image = []
    for i in range(b):
        segs = []
        for _ in range(int(rng.integers(1, 31))):
            a, e, dot, label = point(rng, h, w), point(rng, h, w), rng.random() < 0.2, int(rng.integers(0, 2))
            segs.append((*a, *(a if dot else e), label))
        per_image.append([] if i == empty else segs)
    return dict(params=dict(radius=radius), masks=rng.integers(0, 4, (b, h, w)).astype(np.uint8), per_image=per_image)


def gen_polygons(rng, b, h, w, empty):
    """The packed arrays are built here and not by pack_polygons, whose order (lassos, foreground, background) is one of many."""
    verts, poly_ptr, labels, image_ptr = [], [0], [], [0]
    for i in range(b):
        for _ in range(int(rng.integers(1, 6))):
            v = [point(rng, h, w) for _ in range(int(rng.integers(3, 9)))]
            label = int(rng.integers(0, 3))
            if i != empty:
                verts += v
                poly_ptr.append(poly_ptr[-1] + len(v))
                labels.append(label)
        image_ptr.append(len(labels))
    poison, masks = _masks(rng, b, h, w)
    packed = (np.asarray(verts, np.int32).reshape(-1, 2), np.asarray(poly_ptr, np.int32), np.asarray(labels, np.int32),
              np.asarray(image_ptr, np.int32))
    return dict(params=dict(polygons=len(labels), poison=poison), masks=masks, packed=packed)


def gen_scissors(rng, b, h, w, empty):
    setting = (int(rng.choice([0, 1, 16, 40])), int(rng.choice([1, 300, 2048, 13770])), int(rng.choice([1, 16, 64])))
    kind, imgs = draw_images(rng, b, h, w)
    paths = []
    for i in range(b):
        mine = []
        for _ in range(int(rng.integers(1, 4))):
            closed = bool(rng.random() < 0.5)
            pts = [anchor(rng, h, w) for _ in range(int(rng.integers(3 if closed else 2, 7)))]
            for j in range(1, len(pts)):
                if rng.random() < 0.15:
                    pts[j] = pts[j - 1]                                 # a repeated anchor: a segment without pixels
            mine.append((pts, closed))
        paths.append(None if i == empty else mine)
    return dict(params=dict(margin=setting[0], edge_cap=setting[1], smooth=setting[2], image_kind=kind), imgs=imgs,
                paths=paths, setting=setting)


def _blobs(rng, h, w):
    return click_tests.blobs(rng, h, w, int(rng.integers(1, 4)))


def gen_next_click(rng, b, h, w, empty):
    scale = int(rng.choice([1, 255]))
    preds, gts = [], []
    for i in range(b):
        gt = _blobs(rng, h, w)
        pred = (gt & ~_blobs(rng, h, w)) | _blobs(rng, h, w)
        preds.append((gt if i == empty else pred).astype(np.uint8))     # the image without an error: no click
        gts.append(gt.astype(np.uint8) * scale)
    return dict(params=dict(gt_scale=scale), preds=np.stack(preds), gts=np.stack(gts))


def gen_clean(rng, b, h, w, empty):
    density = float(rng.choice([0.05, 0.3, 0.6]))
    masks = (rng.random((b, h, w)) < density).astype(np.uint8)
    if empty is not None:
        masks[empty] = 0
    return dict(params=dict(density=density), masks=masks)


def gen_eval_counts(rng, b, h, w, empty):
    width, with_trimap = int(rng.choice([0, 1, 3])), bool(rng.random() < 0.6)
    gt = np.stack([_blobs(rng, h, w) for _ in range(b)])
    pred = np.stack([_blobs(rng, h, w) for _ in range(b)]) ^ (rng.random((b, h, w)) < 0.02)
    tri = rng.integers(0, 4, (b, h, w)).astype(np.uint8)
    return dict(params=dict(width=width, trimap=with_trimap), pred=pred.astype(np.uint8), gt=gt.astype(np.uint8),
                tri=tri if with_trimap else None)


def _levels(rng, h, w):
    kind = int(rng.integers(0, 3))
    rnd = matte_eval_ref.random_levels(rng, h, w)
    blocky = matte_eval_ref.blocky_levels(rng, h, w, int(rng.choice([3, 5])))
    fading = matte_eval_ref.fading_levels(h, w, int(rng.choice([20, 130, 200, 255])))
    return (rnd, blocky, fading)[kind]


def gen_matte(rng, b, h, w, empty):
    with_region = bool(rng.random() < 0.5)
    a = np.stack([_levels(rng, h, w) for _ in range(b)])
    g = np.stack([_levels(rng, h, w) for _ in range(b)])
    region = (rng.random((b, h, w)) < 0.4).astype(np.uint8) * rng.integers(1, 256, (b, h, w)).astype(np.uint8)
    return dict(params=dict(region=with_region), a=a, g=g, region=region if with_region else None)


def gen_seed_prior(rng, b, h, w, empty):
    """Trimaps without foreground, without background, or with both (left alone); priors on a grid of 1/4 in half of the
    cases, so that the top-k selection meets ties."""
    frac, coarse = float(rng.choice([0.1, 0.25])), bool(rng.random() < 0.5)
    segs = _segments(rng, b, h, w)
    node_ptr = np.concatenate([[0], np.cumsum([int(s.max()) + 1 for s in segs])]).astype(np.int32)
    prior = rng.random((int(node_ptr[-1]), 3)).astype(np.float32)
    mixed = rng.integers(0, 4, (b, h, w)).astype(np.uint8)
    kinds = rng.integers(0, 4, b)
    trimap = np.stack([mixed[i] if kinds[i] == 3 else np.full((h, w), (2, 1, 3)[kinds[i]], np.uint8) for i in range(b)])
    return dict(params=dict(seed_frac=frac, coarse_prior=coarse, trimaps=kinds.tolist()), segs=segs, node_ptr=node_ptr,
                prior=(np.round(prior * 4) / 4).astype(np.float32) if coarse else prior, trimap=trimap)


GENERATORS = dict(clicks=gen_clicks, geodesic=gen_geodesic, strokes=gen_strokes, stroke_pixels=gen_strokes,
                  polygons=gen_polygons, scissors=gen_scissors, next_click=gen_next_click, clean=gen_clean,
                  eval_counts=gen_eval_counts, matte=gen_matte, mask_iou=gen_eval_counts, seed_prior=gen_seed_prior)


def make_case(family, seed, index):
    rng = case_rng(family, seed, index)
    h, w = draw_shape(rng, index, edges_of(family))
    b = int(BATCHES[int(rng.integers(len(BATCHES)))])
    at = int(rng.integers(b))
    empty = at if b >= 3 else None                                      # in a batch of 3 or more one image has no primitives
    case = GENERATORS[family](rng, b, h, w, empty)
    case.update(family=family, seed=int(seed), index=int(index), b=b, h=int(h), w=int(w), empty=empty)
    return case


def make_cases(family, seed, n=N_CASES):
    return [make_case(family, seed, i) for i in range(n)]


def describe(case):
    params = " ".join(f"{k}={v}" for k, v in case["params"].items())
    return f"{case['family']} seed={case['seed']} case={case['index']} {case['b']}x{case['h']}x{case['w']} {params}"


# ---------------------------------------------------------------- layer 2: the references (the restatements, on the CPU)

def _pair(entry):
    return entry if entry is not None else ([], [])


def ref_clicks(case, orc=None):
    from gcn_grabcut.graph_builder import encode_user_hints
    p = case["params"]
    masks, tables = [], []
    for i in range(case["b"]):
        fg, bg = _pair(case["per_image"][i])
        masks.append(hints_tests.paint(case["masks"][i], case["segs"][i], fg, bg, p["radius"], p["region"]))
        tables.append(encode_user_hints(case["segs"][i], fg, bg))
    return dict(mask=np.stack(masks), node_table=np.concatenate(tables))


def geodesic_full(case):
    """All four outputs of every image, whatever subset the case asks the device for."""
    p = case["params"]
    return [geodesic_ref.geodesic_ref(case["imgs"][i], *_pair(case["per_image"][i]), p["radius"], p["gamma"],
                                      mask=case["masks"][i], segments=case["segs"][i]) for i in range(case["b"])]


def ref_geodesic(case, orc=None):
    full = geodesic_full(case)
    out = {k: (np.concatenate if k == "node_dist" else np.stack)([f[k] for f in full]) for k in case["outputs"]}
    out["_full"] = full                                                 # not compared: for the checks of the fuzzer itself
    return out


def stroke_labels(case, radius):
    return np.stack([strokes_ref.labels(case["h"], case["w"], segs, radius) for segs in case["per_image"]])


def ref_strokes(case, orc=None):
    radius = case["params"]["radius"]
    lab = stroke_labels(case, radius)                                   # strokes_ref.paint is these labels laid over the mask
    return dict(mask=np.where(lab >= 0, lab, case["masks"]).astype(np.uint8),
                poisoned=np.where(lab >= 0, lab, POISON).astype(np.uint8))


def ref_stroke_pixels(case, orc=None):
    rows = [strokes_ref.pixels(case["h"], case["w"], segs) for segs in case["per_image"]]
    lab = stroke_labels(case, 0)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return dict(hint_ptr=ptr, fill_ptr=ptr, rows=np.concatenate(rows), spare_row=np.full(3, -9, np.int32),
                painted_by_hints=np.where(lab >= 0, lab, POISON).astype(np.uint8))


def ref_polygons(case, orc=None):
    return dict(mask=polygons_ref.apply_packed(case["masks"], *case["packed"]))


def path_image_ptr(paths):
    return np.concatenate([[0], np.cumsum([len(p or []) for p in paths])]).astype(np.int32)


def ref_scissors(case, orc=None):
    planes = []
    verts, ptr = scissors_ref.trace_batch(list(case["imgs"]), case["paths"], *case["setting"], planes=planes)
    out = dict(count_ptr=ptr, fill_ptr=ptr, verts=verts, spare_row=np.full(2, scissors_tests.POISON, np.int32),
               planes=np.concatenate(planes).astype(np.int32))
    if (np.diff(ptr) >= 3).all():                                       # the chained case: every traced path is a lasso
        poison = np.full((case["b"], case["h"], case["w"]), POISON, np.uint8)
        out["lassoed"] = polygons_ref.apply_packed(poison, verts, ptr, np.full(len(ptr) - 1, 2, np.int32),
                                                   path_image_ptr(case["paths"]))
    return out


def ref_next_click(case, orc=None):
    return dict(click=np.asarray([click_tests.next_click(p, g) for p, g in zip(case["preds"], case["gts"])], np.int64))


def _rule_key(ratio, keep):
    return f"rule({ratio},{keep})"


def ref_clean(case, orc):
    return {_rule_key(ratio, keep): np.stack([orc.clean_mask(m, ratio, bool(keep)) for m in case["masks"]])
            for ratio, keep in clean_tests.RULES}


def ref_eval_counts(case, orc):
    tri = case["tri"]
    return dict(counts=np.stack([orc.eval_counts(case["pred"][i], case["gt"][i], None if tri is None else tri[i],
                                                 case["params"]["width"]) for i in range(case["b"])]))


def ref_matte(case, orc=None):
    reg = case["region"]
    e = [matte_eval_ref.matte_errors_ref(case["a"][i], case["g"][i], None if reg is None else reg[i]) for i in range(case["b"])]
    return dict(sums=np.asarray([[x[k] for k in matte_tests.INTS] for x in e], np.int64), levels=np.stack([x["levels"] for x in e]),
                grad=np.asarray([x["grad"] for x in e], np.float64))


def ref_mask_iou(case, orc=None):
    """R0 in numpy: tp, fp, fn of pred / gt != 0 and tp / (tp + fp + fn + 1e-8) in float64."""
    p, g = case["pred"].reshape(case["b"], -1) != 0, case["gt"].reshape(case["b"], -1) != 0
    counts = np.stack([(p & g).sum(1), (p & ~g).sum(1), (~p & g).sum(1)], 1).astype(np.int64)
    return dict(counts=counts, iou=counts[:, 0] / (counts.sum(1).astype(np.float64) + 1e-8))


def ref_seed_prior(case, orc):
    n = case["node_ptr"]
    return dict(trimap=np.stack([orc.seed_from_prior(case["trimap"][i], case["prior"][n[i]:n[i + 1]], case["segs"][i],
                                                     case["params"]["seed_frac"]) for i in range(case["b"])]))


REFERENCES = dict(clicks=ref_clicks, geodesic=ref_geodesic, strokes=ref_strokes, stroke_pixels=ref_stroke_pixels,
                  polygons=ref_polygons, scissors=ref_scissors, next_click=ref_next_click, clean=ref_clean,
                  eval_counts=ref_eval_counts, matte=ref_matte, mask_iou=ref_mask_iou, seed_prior=ref_seed_prior)


def reference(case, orc=None):
    """name -> array: what the device must return for this case.  orc: the CPU oracle, for the families that need it."""
    return REFERENCES[case["family"]](case, orc)


_SUITE_CASES = {}          # (family, seed, n) -> the case list
_SUITE_REFERENCES = {}     # (family, seed, n, index) -> the reference of that case


def suite_cases(family, seed, n=N_CASES):
    """The suite's case list of one family and seed, built once per process."""
    if (family, seed, n) not in _SUITE_CASES:
        _SUITE_CASES[family, seed, n] = make_cases(family, seed, n)
    return _SUITE_CASES[family, seed, n]


def suite_reference(family, seed, index, orc=None, n=N_CASES):
    """The reference of one case of the suite's lists, computed once per process and shared by every test that needs it."""
    if (family, seed, n, index) not in _SUITE_REFERENCES:
        _SUITE_REFERENCES[family, seed, n, index] = reference(suite_cases(family, seed, n)[index], orc)
    return _SUITE_REFERENCES[family, seed, n, index]


# ---------------------------------------------------------------- comparison and replay

def compare(case, want, got):
    """-> the mismatch lines of one case (none: it matches).  Exact, but for the two float64 outputs: GRAD within
    test_matte_eval_gpu's GRAD_RTOL, the IoU quotient within test_grabcut_gpu's 1e-12."""
    lines = []
    for key, w in want.items():
        if key.startswith("_"):
            continue
        if key not in got:
            lines.append(f"{describe(case)}: {key} was not produced ({got.get('skipped', 'no reason given')})")
            continue
        w, g = np.asarray(w), np.asarray(got[key])
        if w.shape != g.shape:
            lines.append(f"{describe(case)}: {key} has shape {g.shape}, not {w.shape}")
            continue
        bad = g != w
        if key in ("grad", "iou"):
            bad = np.abs(g - w) > (matte_tests.GRAD_RTOL * (1.0 + w) if key == "grad" else IOU_ATOL)
        if bad.any():
            first = tuple(int(v) for v in np.argwhere(bad)[0])
            lines.append(f"{describe(case)}: {key} differs in {int(bad.sum())} of {bad.size} elements, first at {first} "
                         f"(want {w[first]}, got {g[first]})")
    return lines


# ---------------------------------------------------------------- layer 3: the device runners (the wrappers of the entries' own tests)

class Device:
    """The engine on cuda:0 and its context; made once per pass, so that every case runs on the scratch the last one left."""

    def __init__(self):
        from gcn_grabcut._engine import get_engine
        self.eng = get_engine("cuda")
        self.ctx = self.eng.ctx


def dev_clicks(dev, case, want):
    p = case["params"]
    mask, table, _ = hints_tests._apply(dev.eng, case["masks"], case["segs"], case["per_image"], p["radius"], p["region"])
    return dict(mask=mask, node_table=table)


def dev_geodesic(dev, case, want):
    p = case["params"]
    got = geodesic_tests._call(dev.eng, case["imgs"], case["per_image"], p["radius"], p["gamma"], case["masks"], case["segs"],
                               want=case["outputs"])
    if "node_dist" in got:
        got["node_dist"] = np.concatenate(got["node_dist"])
    return got


def dev_strokes(dev, case, want):
    radius = case["params"]["radius"]
    return dict(mask=stroke_tests._apply(dev.eng, case["masks"], case["per_image"], radius),
                poisoned=stroke_tests._apply(dev.eng, np.full_like(case["masks"], POISON), case["per_image"], radius))


def dev_stroke_pixels(dev, case, want):
    import torch
    eng, shape = dev.eng, (case["b"], case["h"], case["w"])
    counted, rows, fill_ptr, spare = stroke_tests._pixels(eng, shape, case["per_image"], raw=True)
    got = dict(hint_ptr=counted, fill_ptr=fill_ptr, rows=rows, spare_row=spare)
    if not np.array_equal(counted, want["hint_ptr"]) or not np.array_equal(rows, want["rows"]):
        got["skipped"] = "the rows differ, so they were not handed to ggc_apply_hints"
        return got
    mask = torch.full(shape, POISON, dtype=torch.uint8, device=eng.device)               # the chained case: the rows as clicks
    if len(rows):
        eng.apply_hints(mask, *eng.upload_hints(rows, fill_ptr), 0)
    got["painted_by_hints"] = mask.cpu().numpy()
    return got


def dev_polygons(dev, case, want):
    return dict(mask=polygon_tests._apply(dev.eng, case["masks"], case["packed"]))


def scissors_plane_sizes(case):
    sizes = []
    for paths in case["paths"]:
        for pts, closed in paths or []:
            for a, b in scissors_ref.segments(pts, closed):
                _, _, wh, ww = scissors_ref.window(a, b, case["setting"][0], case["h"], case["w"])
                sizes.append(wh * ww)
    return sizes


def dev_scissors(dev, case, want):
    from gcn_grabcut.graph_builder import pack_paths
    eng = dev.eng
    packed = eng.upload_paths(*pack_paths([None if not p else [(a, bool(c)) for a, c in p] for p in case["paths"]]))
    bgr = eng.to_device(np.ascontiguousarray(case["imgs"]))
    count_ptr, fill_ptr, verts, spare = scissors_tests._count_then_fill(eng, bgr, packed, case["setting"])
    planes = np.empty(sum(scissors_plane_sizes(case)), np.int32)
    eng.ctx.call("ggc_debug_read_scratch", b"scissors_planes", planes.ctypes.data, planes.nbytes)
    got = dict(count_ptr=count_ptr, fill_ptr=fill_ptr, verts=verts, spare_row=spare, planes=planes)
    if "lassoed" in want:                                                                # the chained case
        if not np.array_equal(count_ptr, want["count_ptr"]) or not np.array_equal(verts, want["verts"]):
            got["skipped"] = "the vertices differ, so they were not handed to ggc_apply_polygons"
            return got
        masks = np.full((case["b"], case["h"], case["w"]), POISON, np.uint8)
        lassos = (verts, fill_ptr, np.full(len(fill_ptr) - 1, 2, np.int32), path_image_ptr(case["paths"]))
        got["lassoed"] = polygon_tests._apply(eng, masks, lassos)
    return got


def dev_next_click(dev, case, want):
    return dict(click=np.asarray(click_tests.run(list(case["preds"]), list(case["gts"])), np.int64))


def dev_clean(dev, case, want):
    return {_rule_key(ratio, keep): clean_tests._clean(dev.ctx, case["masks"], ratio, keep) for ratio, keep in clean_tests.RULES}


def dev_eval_counts(dev, case, want):
    from gcn_grabcut import metrics
    return dict(counts=metrics._counts(case["pred"], case["gt"], case["tri"], case["params"]["width"], binarize=False))


def dev_matte(dev, case, want):
    sums, grad, levels = matte_tests._call(dev.ctx, case["a"], case["g"], case["region"])
    return dict(sums=sums, grad=grad, levels=levels)


def dev_mask_iou(dev, case, want):
    iou, counts = dev.eng.iou(dev.eng.to_device(case["pred"]), dev.eng.to_device(case["gt"]))
    return dict(counts=counts.cpu().numpy(), iou=iou.cpu().numpy())


def dev_seed_prior(dev, case, want):
    eng = dev.eng
    trimap = eng.to_device(case["trimap"].copy())
    eng.seed_from_prior(trimap, eng.to_device(case["prior"]), eng.to_device(case["node_ptr"]), eng.to_device(case["segs"]),
                        case["params"]["seed_frac"])
    return dict(trimap=trimap.cpu().numpy())


RUNNERS = dict(clicks=dev_clicks, geodesic=dev_geodesic, strokes=dev_strokes, stroke_pixels=dev_stroke_pixels,
               polygons=dev_polygons, scissors=dev_scissors, next_click=dev_next_click, clean=dev_clean,
               eval_counts=dev_eval_counts, matte=dev_matte, mask_iou=dev_mask_iou, seed_prior=dev_seed_prior)


def run_case(dev, case, want):
    """One case on the device -> its mismatch lines.  An entry that refuses or gives up (every input here is valid) is a
    line too, so that it can be replayed, and is kept in GAVE_UP: behind GGC_E_DEVICE may stand a fault of the card, so
    callers end their pass there and start nothing more on the context.  Any other exception is not caught."""
    from gcn_grabcut._native import GGCError
    try:
        return compare(case, want, RUNNERS[case["family"]](dev, case, want))
    except GGCError as e:
        GAVE_UP.append(f"{describe(case)}: {REFUSED} {e}")
        return GAVE_UP[-1:]


def run_family(dev, family, seed, orc=None, n=N_CASES):
    """The suite's cases of one family -> their mismatch lines; the pass ends at the first case whose entry gave up."""
    lines = []
    for i in range(n):
        lines += run_case(dev, suite_cases(family, seed, n)[i], suite_reference(family, seed, i, orc, n))
        if lines and REFUSED in lines[-1]:
            break
    return lines


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--family", choices=FAMILIES)
    ap.add_argument("--seed", type=int, default=int(os.environ.get("FUZZ_SEED", "1")))
    ap.add_argument("--case", type=int, help="run this case alone")
    args = ap.parse_args(argv)
    from oracle import oracle as orc          # checker
    dev = Device()
    if args.case is not None:
        if args.family is None:
            ap.error("--case needs --family")
        case = make_case(args.family, args.seed, args.case)
        lines = run_case(dev, case, reference(case, orc))
        print("\n".join(lines) if lines else f"{describe(case)}: ok")
        return 1 if lines else 0
    n, bad = int(os.environ.get("FUZZ_N", str(N_CASES))), 0
    for family in ([args.family] if args.family else FAMILIES):
        t0, lines = time.time(), []
        for i in range(n):
            case = make_case(family, args.seed, i)
            lines += run_case(dev, case, reference(case, orc))
            if lines and REFUSED in lines[-1]:
                break
        print("\n".join(lines + [f"{family}: seed {args.seed}, {n} cases, {len(lines)} mismatch lines, {time.time() - t0:.0f} s"]),
              flush=True)
        bad += len(lines)
    print("FUZZ DONE: mismatch lines", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
