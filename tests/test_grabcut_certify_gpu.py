"""Every GrabCut iteration of the device, certified by the float64 GrabCut of tests/grabcut_ref.py.

ggc_grabcut runs with n_iter = 0, 1, ..., 5 from the same start and seed (n_iter = 0 returns the set-up mask and the
k-means models, or the given models in mode 2).  Each step (models_{k-1}, mask_{k-1}) -> (models_k, mask_k) must pass
grabcut_ref.certify_step: models equal to learn(assign(models_{k-1})) to rtol 1e-12, probable pixels equal to the
canonical cut of the reference network, energy within the quantisation bound.  For k >= 2 this certifies the warm-started
solves on GrabCut's own networks.  Per-image seeds are seed + b, as in test_grabcut_gpu.py."""
import numpy as np
import pytest

import grabcut_ref as gr
from test_grabcut_gpu import _grabcut, _trimaps

pytestmark = pytest.mark.gpu
N_ITER = 5
SEED = 11


def _run(ctx, imgs, st, k, seed=SEED):
    b = len(imgs)
    masks = None if st["mode"] == 1 else np.stack([st["mask"]] * b) if st["mask"].ndim == 2 else st["mask"]
    rects = None if st["mode"] != 1 else [st["rect"]] * b
    bgd = fgd = None
    if st["mode"] == 2:
        bgd, fgd = np.stack([st["bgd"]] * b), np.stack([st["fgd"]] * b)
    _, m, bg, fg = _grabcut(ctx, imgs, masks, n_iter=k, mode=st["mode"], rects=rects, seed=seed, bgd=bgd, fgd=fgd)
    return m, bg, fg


def _certify_chain(oracle, ctx, imgs, st, what, n_iter=N_ITER):
    states = [_run(ctx, imgs, st, k) for k in range(n_iter + 1)]
    h, w = imgs.shape[1:3]
    for i in range(len(imgs)):
        m0 = states[0][0][i]
        if st["mode"] == 1:
            assert np.array_equal(m0, gr.init_rect(h, w, st["rect"])), f"{what}[{i}]: rect set-up"
        else:
            mi = st["mask"] if st["mask"].ndim == 2 else st["mask"][i]
            want = mi if st["mode"] == 2 else gr.init_trimap(mi)[0]
            assert np.array_equal(m0, want), f"{what}[{i}]: mask set-up"
        for k in range(1, n_iter + 1):
            gr.certify_step(oracle, imgs[i], *(s[i] for s in states[k - 1]), *(s[i] for s in states[k]),
                            what=f"{what}[{i}] it{k}", exact_ties=st["exact_ties"])
    return states


@pytest.mark.parametrize("family,variant", gr.cases())
def test_family_iterations_certified(oracle, gpu_ctx, family, variant):
    st = gr.make(family, variant, seed=3)
    _certify_chain(oracle, gpu_ctx, st["img"][None], st, f"{family}/{variant}")


@pytest.mark.parametrize("h,w,b", [(48, 64, 3), (96, 128, 2), (200, 272, 2), (300, 400, 2)])
def test_synthetic_iterations_certified(oracle, gpu_ctx, h, w, b):
    from gcn_grabcut.synthetic import synthetic_image
    pairs = [synthetic_image(h, w, 7300 + i, return_mask=True) for i in range(b)]
    imgs = np.stack([p[0] for p in pairs])
    tris = _trimaps(imgs, [p[1] for p in pairs])
    st = dict(mode=0, mask=tris, rect=None, exact_ties=False)
    _certify_chain(oracle, gpu_ctx, imgs, st, f"synthetic {h}x{w}")


def test_full_hd_first_iteration_certified(oracle, gpu_ctx):
    from gcn_grabcut.synthetic import synthetic_image
    img, gt = synthetic_image(1080, 1920, 7400, return_mask=True)
    tri = _trimaps(img[None], [gt])
    st = dict(mode=0, mask=tri, rect=None, exact_ties=False)
    _certify_chain(oracle, gpu_ctx, img[None], st, "1080x1920", n_iter=1)


def test_eval_mode_chain_certified(oracle, gpu_ctx):
    """mode 2 calls that feed the models back, one iteration each, certified and equal to one call of n_iter = 4."""
    for family, variant in (("underflow", "one_side"), ("near_lambda", "sweep"), ("singular", "few_colours")):
        st = gr.make(family, variant, seed=3)
        img = st["img"][None]
        m, bg, fg = _run(gpu_ctx, img, st, 0)
        for k in range(1, 5):
            _, m1, bg1, fg1 = _grabcut(gpu_ctx, img, m, n_iter=1, mode=2, bgd=bg, fgd=fg)
            gr.certify_step(oracle, st["img"], m[0], bg[0], fg[0], m1[0], bg1[0], fg1[0], what=f"{family} eval {k}",
                            exact_ties=st["exact_ties"])
            m, bg, fg = m1, bg1, fg1
        m4, bg4, fg4 = _run(gpu_ctx, img, st, 4)
        assert np.array_equal(m, m4) and np.array_equal(bg, bg4) and np.array_equal(fg, fg4), family


def test_degenerate_trimaps_batched_with_normal_images(oracle, gpu_ctx):
    """Skipped images keep their (promoted) trimap and do not disturb the others, which are certified."""
    from gcn_grabcut.synthetic import synthetic_image
    pairs = [synthetic_image(48, 64, 7500 + i, return_mask=True) for i in range(4)]
    imgs = np.stack([p[0] for p in pairs])
    tris = _trimaps(imgs, [p[1] for p in pairs])
    tris[1] = gr.GC_PR_BGD                                    # one class only: promoted to all background, skipped
    tris[2] = np.where(tris[2] == gr.GC_FGD, gr.GC_FGD, gr.GC_PR_FGD)    # foreground labels only: skipped
    st = dict(mode=0, mask=tris, rect=None, exact_ties=False)
    states = [_run(gpu_ctx, imgs, st, k) for k in range(3)]
    for i in (1, 2):
        want, degenerate = gr.init_trimap(tris[i])
        assert degenerate
        for m, _, _ in states:
            assert np.array_equal(m[i], want), i
    for i in (0, 3):
        for k in (1, 2):
            gr.certify_step(oracle, imgs[i], *(s[i] for s in states[k - 1]), *(s[i] for s in states[k]),
                            what=f"batch[{i}] it{k}")
        _, wm, wb, wf, rc = oracle.grabcut(imgs[i], tris[i], n_iter=2, mode=0, seed=SEED + i)
        assert rc == 0 and np.array_equal(states[2][0][i], wm) and np.array_equal(states[2][1][i], wb)
