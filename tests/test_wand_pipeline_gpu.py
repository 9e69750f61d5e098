"""The magic wand through the Python layers on the MI355X, on one small synthetic scene: a flat backdrop with noise of an
amplitude below the tolerance, and a textured square on it.  The public functions against tests/wand_ref.py, the pipeline
with wand seeds (hard constraints, paint order, batches), GrabCut.add_wand / run_with_wand, and the chain into a matte."""
import dataclasses

import numpy as np
import pytest

import wand_ref as ref
from helpers import seeded_state_dict

pytestmark = pytest.mark.gpu
H, W = 72, 96
TOL = 12                                    # the backdrop's noise is 0..5 per byte: every backdrop pixel is within 5 of every other
SQUARE = (slice(20, 52), slice(30, 70))
CORNER, INSIDE = (0, 0), (36, 50)


def scene(seed=0):
    """Backdrop (60, 90, 120) + 0..5 noise; the square holds bytes in 150..255, at least 25 from the backdrop in every channel."""
    rng = np.random.default_rng(seed)
    img = np.array([60, 90, 120], np.uint8)[None, None, :] + rng.integers(0, 6, (H, W, 3)).astype(np.uint8)
    img[SQUARE] = rng.integers(150, 256, (32, 40, 3)).astype(np.uint8)
    return np.ascontiguousarray(img)


def backdrop():
    m = np.ones((H, W), bool)
    m[SQUARE] = False
    return m


@pytest.fixture(scope="module")
def wand():
    from gcn_grabcut import Wand
    return Wand(TOL)


@pytest.fixture(scope="module")
def pipe():
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig
    model, sd = seeded_state_dict(32, 2, seed=5)
    return GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=80), device="cuda")


def test_public_functions_equal_the_reference(wand):
    import gcn_grabcut as g
    img = scene()
    _, want, _ = ref.wand_image(img, [(*CORNER, 1)], TOL, 8, 1)
    assert np.array_equal(want != 0, backdrop())                                    # the scene is what it claims
    assert np.array_equal(g.wand_select(img, [CORNER], wand=wand), want)
    for w, seeds in ((g.Wand(TOL, 4, True, 3), [(*INSIDE, 1), (*CORNER, 0)]), (g.Wand(60, 8, False, 5), [(*CORNER, 1), (21, 31, 1), (*INSIDE, 0)])):
        fg, bg = [s[:2] for s in seeds if s[2]], [s[:2] for s in seeds if not s[2]]
        start = np.random.default_rng(3).integers(0, 4, (H, W)).astype(np.uint8)
        m, s, c = ref.wand_image(img, seeds, *w.args(), start)
        assert np.array_equal(g.wand_select(img, fg, bg, w), s)
        assert np.array_equal(g.paint_wand(start, img, fg, bg, w), m)
        sel, cnt = g.wand_select_batch([img, scene(1)], [(fg, bg), None], w, return_counts=True)
        assert np.array_equal(sel[0], s) and not sel[1].any() and cnt.tolist() == [c.tolist(), [0, 0]]
    assert np.array_equal(g.paint_wand((H, W), img, [], [CORNER], wand), np.where(backdrop(), 0, 2))


def test_segment_keeps_a_background_selection_out_of_the_mask(pipe, wand):
    img = scene()
    r = pipe.segment(img, bg_wand=[CORNER], wand=wand, min_area_ratio=0.0)
    assert (r.trimap[backdrop()] == 0).all() and not r.binary_mask[backdrop()].any()
    plain = pipe.segment(img, min_area_ratio=0.0)
    empty = pipe.segment(img, min_area_ratio=0.0, fg_wand=(), bg_wand=())
    for k in ("binary_mask", "trimap", "segments", "overlay", "rgba"):
        assert getattr(empty, k).tobytes() == getattr(plain, k).tobytes(), k         # no seed: the call without the argument
    assert np.array_equal(r.trimap[SQUARE], plain.trimap[SQUARE])                   # undecided pixels keep the network's label


def test_paint_order_polygons_then_wands_then_clicks(pipe, wand):
    img = scene()
    bgr = pipe._eng.to_device(img[None])
    click = (5, 80)
    yy, xx = np.mgrid[0:H, 0:W]
    disk = (yy - click[0]) ** 2 + (xx - click[1]) ** 2 <= 9
    out = pipe.segment_batch_device(bgr, chunks=1, min_area_ratio=0.0, wands=[([], [CORNER])], wand=wand,
                                    hints=[([click], [])], hint_radius=3)
    tri = out["trimap"][0].cpu().numpy()
    assert (tri[disk] == 1).all() and (tri[backdrop() & ~disk] == 0).all()          # the click survives inside the selection
    gc_mask = out["gc_mask"][0].cpu().numpy()
    assert (gc_mask[disk] == 1).all() and (gc_mask[backdrop() & ~disk] == 0).all()
    fill = [(60, 5), (60, 40), (70, 40), (70, 5)]                                   # a background fill on the backdrop
    out = pipe.segment_batch_device(bgr, chunks=1, min_area_ratio=0.0, polygons=[([], [fill], [])], wands=[([CORNER], [])], wand=wand)
    tri = out["trimap"][0].cpu().numpy()
    assert (tri[backdrop()] == 1).all()                                             # the wand's selection is painted over the fill
    only = pipe.segment_batch_device(bgr, chunks=1, min_area_ratio=0.0, polygons=[([], [fill], [])])["trimap"][0].cpu().numpy()
    assert (only[60:71, 5:41] == 0).all() and np.array_equal(only[SQUARE], tri[SQUARE])


def test_batch_equals_per_image_segment(pipe, wand):
    from gcn_grabcut import GCNGrabCutPipeline
    imgs = [scene(0), scene(1), scene(2)]
    wands = [([], [CORNER]), None, ([INSIDE], [CORNER, (71, 95)])]
    res = pipe.segment_batch(imgs, wands=wands, wand=wand, min_area_ratio=0.0, chunks=1)
    for i, (img, seeds) in enumerate(zip(imgs, wands)):                              # image i of a batch cuts with seed + i
        one = GCNGrabCutPipeline(pipe.model, sp_config=pipe.sp_config, device="cuda",
                                 gc_config=dataclasses.replace(pipe.gc_config, seed=pipe.gc_config.seed + i))
        fg, bg = seeds if seeds is not None else (None, None)
        r = one.segment(img, fg_wand=fg, bg_wand=bg, wand=wand, min_area_ratio=0.0)
        for k in ("trimap", "segments", "binary_mask"):
            assert np.array_equal(getattr(res[i], k), getattr(r, k)), (i, k)
    assert not res[0].binary_mask[backdrop()].any() and not res[2].binary_mask[backdrop()].any()
    four = imgs + [scene(3)]
    wands4 = wands + [([], [CORNER])]
    bgr = pipe._eng.to_device(np.stack(four))
    a = pipe.segment_batch_device(bgr, chunks=1, min_area_ratio=0.0, wands=wands4, wand=wand)
    b = pipe.segment_batch_device(bgr, chunks=2, min_area_ratio=0.0, wands=wands4, wand=wand)
    for k in ("binary_mask", "trimap", "gc_mask"):
        assert np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), k              # chunks carry their own seeds


def test_grabcut_add_wand_and_run_with_wand(pipe, wand):
    from gcn_grabcut import GrabCut, Wand
    img = scene()
    gc = GrabCut(img, device="cuda")
    with pytest.raises(RuntimeError):
        gc.add_wand(bg_points=[CORNER], wand=wand)
    tri = np.full((H, W), 2, np.uint8)
    tri[10:62, 20:80] = 3
    tri[30:40, 40:60] = 1
    tri[:3] = 0
    gc.run_with_trimap(tri)
    m0 = gc.mask.copy()
    gc.add_wand(bg_points=[CORNER], wand=wand)
    want, _, _ = ref.wand_image(img, [(*CORNER, 0)], TOL, 8, 1, m0)
    assert np.array_equal(gc.mask, want) and gc.history[-1].tag == "wand"
    binary = gc.refine(1)
    assert (gc.mask[backdrop()] == 0).all() and not binary[backdrop()].any()        # refine keeps the painted pixels
    gc2 = GrabCut(img, device="cuda")
    binary = gc2.run_with_wand([CORNER], wand=wand)
    assert not binary[backdrop()].any() and binary.any()
    assert np.array_equal(gc2.wand_trimap([CORNER], [INSIDE], Wand(0)),
                          np.where(ref.selection(img, *CORNER, 0, 8, 1), 0, np.where(ref.selection(img, *INSIDE, 0, 8, 1), 1, 3)))
    r = pipe.segment_wand(img, [CORNER], wand=wand)
    assert np.array_equal(r.binary_mask, binary) and np.array_equal(r.trimap, np.where(backdrop(), 0, 3))
    with pytest.raises(ValueError, match="no background"):
        gc2.run_with_wand([(H, W)], wand=wand)                                       # the only seed lies outside: nothing selected
    with pytest.raises(ValueError, match="no background"):
        gc2.run_with_wand([], [INSIDE], wand=wand)
    with pytest.raises(ValueError, match="every pixel"):
        gc2.run_with_wand([CORNER], wand=Wand(255))
    with pytest.raises(ValueError, match="every pixel"):
        pipe.segment_wand(img, [CORNER], wand=Wand(255))


def test_selection_to_trimap_to_matte_runs_end_to_end(wand):
    import gcn_grabcut as g
    img = scene()
    selection = g.wand_select(img, [CORNER], wand=wand)
    trimap = g.mask_to_trimap(255 - selection, 2, 2)
    assert set(np.unique(trimap)) == {0, 128, 255}
    alpha = g.trimap_matte(img, trimap)
    from gcn_grabcut.pipeline import alpha_to_u8
    assert alpha.shape == (H, W) and np.isfinite(alpha).all()
    a8 = alpha_to_u8(alpha)
    assert (a8[trimap == 255] == 255).all() and (a8[trimap == 0] == 0).all()        # the cut-out keeps the square, drops the backdrop
