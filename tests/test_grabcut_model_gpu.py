"""The GrabCut model kernels (k-means, GMM assignment and learning, beta, mask flags, graph build) at the shapes where
their four-pixel loads can go wrong, scored against oracle.grabcut bit for bit: final mask, both 65-double models, binary
mask.

A thread of these kernels owns four consecutive pixels whose first flat index b P + p is a multiple of 4; whole quads are
dword loads, an image's first and last quad are byte loads.  So the shapes are P % 4 = 1, 2, 3 and P < 4, P around the
1024-pixel k-means chunk, and a width that leaves a partial quad at every row end; every shape runs at batch 3 with
three different images, so that images 1 and 2 start at other byte alignments than image 0.  n_iter 3 reaches the
iterations in which k_gmm_accum<1> takes the component of a probable pixel from the byte k_build_graph left (n_iter 1
never does).  The start states of grabcut_ref.cases() run once each as well."""
import numpy as np
import pytest

import grabcut_ref as gr

SHAPES = [(1, 1), (1, 3), (3, 5), (7, 9), (5, 13), (33, 31), (32, 32), (25, 41), (17, 23)]
DEGENERATE_AT = (17, 23)        # image 1 of this batch is one class only: skipped (state = 1)
SMALL_CLASS_AT = (25, 41)       # image 2 of this batch has a three-pixel foreground class: K = 3 < 5
SEED = 23
_memo = {}


def _trimap(h, w, gt):
    """trimap_of, and below 150 pixels (where its border and core leave nothing probable) a definite first row and centre."""
    if h * w >= 150:
        return gr.trimap_of(gt)
    t = np.where(gt == 1, gr.GC_PR_FGD, gr.GC_PR_BGD).astype(np.uint8)
    t[0] = gr.GC_BGD
    t[h // 2, w // 2] = gr.GC_FGD
    if h * w >= 15:
        t[h // 2, (w // 2 + 1) % w] = gr.GC_PR_FGD
    return t


def _batch(h, w):
    """Three different scenes with their trimaps (mode 0), rects (mode 1) and random masks with hand-made models (mode 2)."""
    if (h, w) in _memo:
        return _memo[h, w]
    rng = np.random.default_rng(1000 * h + w)
    imgs, tris = [], []
    for i in range(3):
        img, gt = gr._blobs(h, w, rng)
        imgs.append(img); tris.append(_trimap(h, w, np.roll(gt, 1 + i, axis=1)))     # off the object: the cut has work to do
    if (h, w) == DEGENERATE_AT:
        tris[1] = np.full((h, w), gr.GC_PR_BGD, np.uint8)
    if (h, w) == SMALL_CLASS_AT:
        t = np.full((h, w), gr.GC_PR_BGD, np.uint8)
        t[:2] = gr.GC_BGD
        t[10, 20] = gr.GC_FGD; t[10, 21] = gr.GC_PR_FGD; t[11, 20] = gr.GC_PR_FGD
        tris[2] = t
    imgs, tris = np.stack(imgs), np.stack(tris)
    rects = np.array([[w // 4, h // 4, max(1, w // 2), max(1, h // 2)], [0, 0, w, max(1, h - 1)], [-2, 1, w // 2 + 2, h]], np.int32)
    masks2 = rng.integers(0, 4, (3, h, w)).astype(np.uint8)
    bgd = gr.model([(0.6, (60, 60, 60), (900.0, 700.0, 800.0)), (0.4, (200, 80, 30), (400.0, 500.0, 300.0))])
    fgd = gr.model([(0.7, (150, 170, 190), (600.0, 600.0, 600.0)), (0.3, (90, 200, 120), (300.0, 800.0, 500.0))])
    _memo[h, w] = dict(imgs=imgs, tris=tris, rects=rects, masks2=masks2, bgd=np.stack([bgd] * 3), fgd=np.stack([fgd] * 3))
    return _memo[h, w]


def _want(orc, bt, mode, n_iter):
    """The oracle's (binary, mask, bgd, fgd, rc) per image; the per-image seed is SEED + b, as on the device."""
    key = ("want", bt["imgs"].shape, mode, n_iter)
    if key not in _memo:
        out = []
        for i in range(3):
            if mode == 0:
                out.append(orc.grabcut(bt["imgs"][i], bt["tris"][i], n_iter=n_iter, mode=0, seed=SEED + i))
            elif mode == 1:
                out.append(orc.grabcut(bt["imgs"][i], None, n_iter=n_iter, mode=1, rect=bt["rects"][i], seed=SEED + i))
            else:
                out.append(orc.grabcut(bt["imgs"][i], bt["masks2"][i], n_iter=n_iter, mode=2, bgd=bt["bgd"][i], fgd=bt["fgd"][i]))
        _memo[key] = out
    return _memo[key]


def _set_up_mask(bt, mode, i):
    h, w = bt["imgs"].shape[1:3]
    if mode == 0:
        return gr.init_trimap(bt["tris"][i])[0]
    return gr.init_rect(h, w, bt["rects"][i]) if mode == 1 else bt["masks2"][i]


def test_the_small_shapes_are_not_all_degenerate(oracle):
    """On the CPU: from 7x9 on every mode-0 batch has images that run the solve, and the solve moves their masks."""
    for h, w in SHAPES:
        if h * w < 63:
            continue
        bt = _batch(h, w)
        want = _want(oracle, bt, 0, 3)
        ran = [i for i in range(3) if want[i][4] == 0]
        assert len(ran) >= (2 if (h, w) == DEGENERATE_AT else 3), (h, w, ran)
        for i in ran:                                            # every image that runs the solve: its result is not its input
            assert not np.array_equal(want[i][1], bt["tris"][i]), (h, w, i)
    assert _want(oracle, _batch(*DEGENERATE_AT), 0, 3)[1][4] == 1
    t = _batch(*SMALL_CLASS_AT)["tris"][2]
    assert 0 < int(gr.is_fg(t).sum()) < 5


@pytest.mark.gpu
@pytest.mark.parametrize("n_iter", [1, 3])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("h,w", SHAPES)
def test_model_kernels_bit_exact(oracle, gpu_ctx, h, w, mode, n_iter):
    from test_grabcut_gpu import _grabcut
    bt = _batch(h, w)
    want = _want(oracle, bt, mode, n_iter)
    masks = bt["tris"] if mode == 0 else (None if mode == 1 else bt["masks2"])
    binary, mask, bgd, fgd = _grabcut(gpu_ctx, bt["imgs"], masks, n_iter=n_iter, mode=mode, seed=SEED,
                                      rects=bt["rects"] if mode == 1 else None,
                                      bgd=bt["bgd"] if mode == 2 else None, fgd=bt["fgd"] if mode == 2 else None)
    for i in range(3):
        wb, wm, wbgd, wfgd, rc = want[i]
        what = (h, w, mode, n_iter, i)
        if rc:                                                   # skipped: the set-up mask, the models untouched
            wm = _set_up_mask(bt, mode, i)
            assert np.array_equal(mask[i], wm), what
            assert np.array_equal(binary[i], gr.is_fg(wm).astype(np.uint8)), what
            assert not bgd[i].any() and not fgd[i].any(), what
            continue
        assert np.array_equal(mask[i], wm), (what, int((mask[i] != wm).sum()))
        assert np.array_equal(binary[i], wb), what
        assert np.array_equal(bgd[i], wbgd) and np.array_equal(fgd[i], wfgd), what


@pytest.mark.gpu
@pytest.mark.parametrize("family,variant", gr.cases())
def test_family_starts_bit_exact(oracle, gpu_ctx, family, variant):
    from test_grabcut_gpu import _grabcut
    st = gr.make(family, variant, seed=3)
    img = st["img"]
    kw = dict(n_iter=3, mode=st["mode"], seed=SEED)
    wb, wm, wbgd, wfgd, rc = oracle.grabcut(img, st["mask"], rect=st["rect"], bgd=st.get("bgd"), fgd=st.get("fgd"), **kw)
    assert rc == 0, (family, variant)
    binary, mask, bgd, fgd = _grabcut(gpu_ctx, img[None], None if st["mask"] is None else st["mask"][None],
                                      rects=None if st["rect"] is None else [st["rect"]],
                                      bgd=None if st["mode"] != 2 else st["bgd"][None],
                                      fgd=None if st["mode"] != 2 else st["fgd"][None], **kw)
    assert np.array_equal(mask[0], wm), int((mask[0] != wm).sum())
    assert np.array_equal(binary[0], wb)
    assert np.array_equal(bgd[0], wbgd) and np.array_equal(fgd[0], wfgd)


def _zero_score_scene():
    """Two probable pixels of a colour C that scores exactly 0 under every component of both models, in every iteration:
    the background is A / A + (2, 0, 0) noise (variance 1 along the first channel, C is 80 away), and the foreground
    component the two pixels are learned into holds 3400 flat pixels beside them, which puts their exponent at about
    -3402 / 4, below the -745.2 under which det_exp is 0.  gmm_which's rule then names component 0 (start at 0 with 0.0,
    strict >), and so must the byte k_build_graph leaves for the next iteration's k_gmm_accum<1>."""
    rng = np.random.default_rng(5)
    h, w = 72, 112
    A, F, C = np.array([40, 60, 80]), np.array([200, 200, 40]), np.array([120, 10, 250])
    img = np.zeros((h, w, 3), np.uint8)
    img[:] = A
    img[rng.random((h, w)) < 0.5] = A + np.array([2, 0, 0])
    mask = np.zeros((h, w), np.uint8)
    img[2:70, 60:110] = F
    mask[2:70, 60:110] = gr.GC_FGD
    for y, x in ((20, 20), (40, 33)):
        img[y, x] = C
        mask[y, x] = gr.GC_PR_FGD
    bgd = gr.model([(0.9, A, (4.0, 4.0, 4.0)), (0.1, 255 - A, (4.0, 4.0, 4.0))])
    fgd = gr.model([(1.0, F, (1.0, 1.0, 1.0))])
    return img, mask, bgd, fgd


def test_zero_score_scene_scores_zero(oracle):
    """On the CPU: after each of three iterations both probable pixels score 0 under all components of both models."""
    img, mask, bgd, fgd = _zero_score_scene()
    px = img[mask >= 2].reshape(-1, 3)
    for n_iter in (1, 2, 3):
        _, m, b, f, rc = oracle.grabcut(img, mask, n_iter=n_iter, mode=2, bgd=bgd, fgd=fgd)
        assert rc == 0
        for model in (b, f):
            assert not gr.scores(model, px, flush_below=-745.2)[0].any(), n_iter


@pytest.mark.gpu
def test_all_zero_scores_take_component_zero(oracle, gpu_ctx):
    from test_grabcut_gpu import _grabcut
    img, mask, bgd, fgd = _zero_score_scene()
    wb, wm, wbgd, wfgd, rc = oracle.grabcut(img, mask, n_iter=3, mode=2, bgd=bgd, fgd=fgd)
    binary, m, b, f = _grabcut(gpu_ctx, img[None], mask[None], n_iter=3, mode=2, bgd=bgd[None], fgd=fgd[None])
    assert np.array_equal(m[0], wm) and np.array_equal(binary[0], wb)
    assert np.array_equal(b[0], wbgd) and np.array_equal(f[0], wfgd)
