"""experiment helper: one digest per seeded case of every entry that csrc/ggc_cg.h, csrc/ggc_cg_compact.h and
csrc/ggc_image.h serve, over the raw outputs, iters and rel_residual.  Run it once per library (GGC_HIP_LIBRARY selects one
per process) and compare the lines: two libraries that compute the same bits print the same text.

Entries: ggc_closed_form_matte, ggc_trimap_matte (with and without alpha0), ggc_trimap_matte_warm, ggc_estimate_foreground,
ggc_poisson_clone (source and mixed gradients; composite, raw, n_omega, iters and rel), ggc_lift_trimap,
ggc_closed_form_band, ggc_alpha_matte, ggc_upsample_matte, ggc_lift_labels, and ggc_refine_trimap in its fused
(radius <= 8) and unfused forms.  The solver batches hold images with nothing to solve (no unknown pixel, every pixel
unknown) between images that are solved."""
import hashlib
import sys
from pathlib import Path

root = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(root))
sys.path.insert(0, str(root / "src"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gcn_grabcut import _native  # noqa: E402
from gcn_grabcut.synthetic import synthetic_image  # noqa: E402

ctx = _native.get_context(0)
H, W, H1, W1 = 70, 90, 151, 187


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def call(name, *args):
    ctx.call(name, _native.current_stream(0), *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])
    torch.cuda.synchronize()


def report(what, *outs):
    h = hashlib.sha256()
    for o in outs:
        h.update(o.cpu().numpy().tobytes())
    print(f"{what}: {h.hexdigest()[:32]}", flush=True)


def empty(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


def matte_outputs(b, h, w):
    return [empty(b, h, w), empty(b, h, w, 4, dtype=torch.uint8), empty(b, h, w, dtype=torch.float64),
            empty(b, dtype=torch.int32), empty(b, dtype=torch.float64)]


rng = np.random.default_rng(10)
pairs = [synthetic_image(H, W, 300 + j, return_mask=True) for j in range(5)]
imgs = np.stack([p[0] for p in pairs])
masks = np.stack([p[1] for p in pairs]).astype(np.uint8)
masks[1] = 0                                                     # no edge: nothing to solve
masks[3] = 1
bgr, binary = dev(imgs), dev(masks)
B = len(imgs)

for r in (1, 2, 3):
    for band in (1, 3):
        out = matte_outputs(B, H, W)
        call("ggc_closed_form_matte", B, H, W, bgr, binary, r, 1e-5, band, 300, 1e-5, *out)
        report(f"closed_form_matte r={r} band={band} iters {out[3].tolist()}", *out)

for band in (0, 2, 5):
    tri = empty(B, H, W, dtype=torch.uint8)
    call("ggc_closed_form_band", B, H, W, binary, band, tri)
    report(f"closed_form_band band={band}", tri)

tri[1] = 128                                                     # every pixel unknown: nothing anchors it
tri[3] = 255
tri[4, H // 2, W // 2] = 7                                       # band 5, and one more unknown byte
alpha0 = dev(rng.uniform(-0.5, 1.5, (B, H, W)).astype(np.float32))
alpha0[0, 3, 4] = float("nan")
for r in (1, 2, 4):
    for name, a0 in (("trimap_matte", None), ("trimap_matte alpha0", alpha0)):
        out = matte_outputs(B, H, W)
        call("ggc_trimap_matte", B, H, W, bgr, tri, r, 1e-5, 300, 1e-5, a0, *out)
        report(f"{name} r={r} iters {out[3].tolist()}", *out)
    warm0 = out[0].clone()                                       # a solved alpha as the warm start
    out = matte_outputs(B, H, W)
    call("ggc_trimap_matte_warm", B, H, W, bgr, tri, r, 1e-5, 300, 1e-4, warm0, *out)
    report(f"trimap_matte_warm r={r} iters {out[3].tolist()}", *out)
    out = matte_outputs(B, H, W)
    call("ggc_trimap_matte_warm", B, H, W, bgr, tri, r, 1e-5, 300, 1e-6, alpha0, *out)
    report(f"trimap_matte_warm from noise r={r} iters {out[3].tolist()}", *out)

alphas = np.stack([np.zeros((H, W)), rng.random((H, W)), np.ones((H, W)),
                   np.clip(rng.normal(0.5, 0.6, (H, W)), -0.5, 1.5), np.zeros((H, W))]).astype(np.float32)
alphas[4, 20:40, 30:50] = rng.random((20, 20))
alphas[3, 0, 0] = np.nan
for eps_r, omega, tol in ((5e-3, 1.0, 1e-6), (1e-2, 0.1, 1e-4)):
    out = [empty(B, H, W, 3, dtype=torch.uint8), empty(B, H, W, 4, dtype=torch.uint8), empty(B, H, W, 3, dtype=torch.float64),
           empty(B, H, W, 3, dtype=torch.float64), empty(B, dtype=torch.int32), empty(B, dtype=torch.float64)]
    call("ggc_estimate_foreground", B, H, W, bgr, dev(alphas), eps_r, omega, 400, tol, *out)
    report(f"estimate_foreground eps_r={eps_r} omega={omega} iters {out[4].tolist()}", *out)

# the clone: a source larger than the target that overhangs it at every offset used; between the solved images an empty
# mask, a mask that covers the target (Omega = the whole target: not solved) and a one-pixel mask
HS, WS = 96, 120
crng = np.random.default_rng(11)
yy, xx = np.mgrid[0:HS, 0:WS]
cmasks = np.stack([(yy - 48) ** 2 + (xx - 60) ** 2 <= 30 ** 2, np.zeros((HS, WS), bool), np.ones((HS, WS), bool),
                   (yy == 40) & (xx == 50), crng.random((HS, WS)) < 0.6, (yy - 30) ** 2 + (xx - 90) ** 2 <= 25 ** 2])
offs = np.array([(-13, -15), (-3, 4), (-20, -25), (-9, -7), (-26, -30), (-40, 10)], np.int32)     # (-40, 10): cut by two borders
BC = len(cmasks)
csrc, ctgt = dev(crng.integers(0, 256, (BC, HS, WS, 3)).astype(np.uint8)), dev(crng.integers(0, 256, (BC, H, W, 3)).astype(np.uint8))
cmask, coff = dev(cmasks.astype(np.uint8) * 255), dev(offs)
for mixed in (0, 1):
    for tol in (1e-7, 1e-4):
        out = [empty(BC, H, W, 3, dtype=torch.uint8), empty(BC, H, W, 3, dtype=torch.float64), empty(BC, dtype=torch.int32),
               empty(BC, dtype=torch.int32), empty(BC, dtype=torch.float64)]
        call("ggc_poisson_clone", BC, HS, WS, csrc, cmask, H, W, ctgt, coff, mixed, 3000, tol, *out)
        report(f"poisson_clone mixed={mixed} tol={tol} n_omega {out[2].tolist()} iters {out[3].tolist()}", *out)

for grow in (0, 3):
    for h1, w1 in ((H1, W1), (H, W), (4 * H, 4 * W)):
        t_full, a_full = empty(B, h1, w1, dtype=torch.uint8), empty(B, h1, w1)
        call("ggc_lift_trimap", B, H, W, tri, alpha0, h1, w1, grow, t_full, a_full)
        report(f"lift_trimap {h1}x{w1} grow={grow}", t_full, a_full)

full = dev(np.stack([synthetic_image(H1, W1, 400 + j) for j in range(B)]))
for r in (1, 4, 40):                                             # 40: windows larger than the image's half, repeated reflection
    a, rgba = empty(B, H, W), empty(B, H, W, 4, dtype=torch.uint8)
    call("ggc_alpha_matte", B, H, W, bgr, binary, r, 1e-4, a, rgba)
    report(f"alpha_matte r={r}", a, rgba)
    a, m, rgba = empty(B, H1, W1), empty(B, H1, W1, dtype=torch.uint8), empty(B, H1, W1, 4, dtype=torch.uint8)
    call("ggc_upsample_matte", B, H, W, bgr, binary, H1, W1, full, r, 1e-4, a, m, rgba)
    report(f"upsample_matte r={r}", a, m, rgba)
full4 = dev(np.stack([synthetic_image(2 * H, 4 * W, 500 + j) for j in range(B)]))    # W1 % 4 == 0: the wide stores
a, m, rgba = empty(B, 2 * H, 4 * W), empty(B, 2 * H, 4 * W, dtype=torch.uint8), empty(B, 2 * H, 4 * W, 4, dtype=torch.uint8)
call("ggc_upsample_matte", B, H, W, bgr, binary, 2 * H, 4 * W, full4, 4, 1e-4, a, m, rgba)
report("upsample_matte r=4 to 140x360", a, m, rgba)

for band in (0, 2, 9):
    labels, m = empty(B, H1, W1, dtype=torch.uint8), empty(B, H1, W1, dtype=torch.uint8)
    call("ggc_lift_labels", B, H, W, binary, H1, W1, band, labels, m)
    report(f"lift_labels band={band}", labels, m)

yy, xx = np.mgrid[0:H, 0:W]
seg = np.broadcast_to(((yy // 5) * -(-W // 7) + xx // 7).astype(np.int32), (B, H, W)).copy()
n = int(seg.max()) + 1
logits = (3 * rng.standard_normal((B * n, 3))).astype(np.float32)
e = np.exp(logits - logits.max(1, keepdims=True))
probs, node_ptr = dev((e / e.sum(1, keepdims=True)).astype(np.float32)), dev(np.arange(B + 1, dtype=np.int32) * n)
for r in (1, 3, 8, 12, 100):                                     # 12, 100: the unfused blurs
    for edge_aware in (1, 0):
        t = empty(B, H, W, dtype=torch.uint8)
        call("ggc_refine_trimap", B, H, W, probs, node_ptr, dev(seg), bgr, 0.55, 0.55, r, 1e-3, edge_aware, t)
        report(f"refine_trimap r={r} edge_aware={edge_aware}", t)
