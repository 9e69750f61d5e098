"""GCNGrabCutPipeline.evaluate_clicks on the MI355X: every image's clicks, GrabCut masks and IoU curve equal a one-image
restatement built from the CPU oracle (scipy next click -> disk -> oracle GrabCut GC_EVAL -> NumPy IoU), stop_iou gives
prefixes of the full run, and segment_batch_device's return_state adds outputs without changing any."""
import numpy as np
import pytest
import torch

from helpers import seeded_state_dict
from test_hints_gpu import paint
from test_next_click_gpu import next_click

pytestmark = pytest.mark.gpu

B, H, W, CLICKS, RADIUS = 8, 72, 104, 5, 3


def np_iou(pred, gt):
    pred, gt = pred != 0, gt != 0
    tp = float((pred & gt).sum())
    fp = float((pred & ~gt).sum())
    fn = float((~pred & gt).sum())
    return tp / ((tp + fp + fn) + 1e-8)


@pytest.fixture(scope="module")
def setup():
    from gcn_grabcut import GCNGrabCutPipeline, SuperpixelGraphConfig
    from gcn_grabcut.synthetic import synthetic_image
    model, _ = seeded_state_dict(32, 2, seed=11)
    pipe = GCNGrabCutPipeline(model.eval(), sp_config=SuperpixelGraphConfig(n_segments=60), device="cuda")
    pairs = [synthetic_image(H, W, 900 + i, return_mask=True) for i in range(B)]
    imgs = [p[0] for p in pairs]
    gts = [p[1] for p in pairs]
    full = pipe.evaluate_clicks(imgs, gts, max_clicks=CLICKS, hint_radius=RADIUS, return_masks=True)
    return pipe, imgs, gts, full


def test_state_is_what_the_edit_loop_continues_from(setup):
    pipe, imgs, gts, full = setup
    bgr = pipe._eng.to_device(np.stack(imgs))
    plain = pipe.segment_batch_device(bgr)
    off = pipe.segment_batch_device(bgr, return_state=False)
    on = pipe.segment_batch_device(bgr, return_state=True)
    assert set(plain) == set(off) and set(on) == set(plain) | {"gc_binary", "bgd", "fgd", "gc_image"}
    for k, v in plain.items():
        if torch.is_tensor(v):
            assert torch.equal(v, off[k]), k
            assert torch.equal(v, on[k]), k
    assert torch.equal(plain["graphs"].x, off["graphs"].x) and torch.equal(plain["graphs"].x, on["graphs"].x)
    assert torch.equal(on["gc_binary"], on["gc_mask"] & 1)
    assert torch.equal(on["gc_image"], bgr)                          # color_space "rgb": GrabCut reads the input itself
    assert on["bgd"].shape == on["fgd"].shape == (B, 65) and on["bgd"].dtype == torch.float64
    four = pipe.segment_batch_device(bgr, chunks=4, return_state=True)    # the software pipeline hands back the same
    for k in ("gc_binary", "gc_mask", "bgd", "fgd", "gc_image", "binary_mask"):
        assert torch.equal(on[k], four[k]), k


def test_each_image_equals_the_one_image_restatement(setup, oracle):
    pipe, imgs, gts, full = setup
    bgr = pipe._eng.to_device(np.stack(imgs))
    st = pipe.segment_batch_device(bgr, return_state=True)
    masks0 = st["gc_mask"].cpu().numpy()
    bgd0, fgd0 = st["bgd"].cpu().numpy(), st["fgd"].cpu().numpy()
    binary0 = st["gc_binary"].cpu().numpy()
    image = st["gc_image"].cpu().numpy()
    assert full["ious"].shape == (B, CLICKS + 1) and full["masks"].shape == (B, CLICKS + 1, H, W)
    moved = 0
    for b in range(B):
        gt = gts[b]
        mask, bgd, fgd, binary = masks0[b], bgd0[b], fgd0[b], binary0[b]
        curve, clicks = [np_iou(binary, gt)], []
        assert np.array_equal(full["masks"][b, 0], mask), b
        for k in range(1, CLICKS + 1):
            r, c, label, _ = next_click(binary, gt)
            if r >= 0:
                clicks.append((r, c, label))
                fg, bg = ([(r, c)], []) if label == 1 else ([], [(r, c)])
                mask = paint(mask, None, fg, bg, RADIUS, False)
            binary, mask, bgd, fgd, _ = oracle.grabcut(image[b], mask, n_iter=1, mode=2, seed=pipe.gc_config.seed,
                                                       bgd=bgd, fgd=fgd)
            curve.append(np_iou(binary, gt))
            assert np.array_equal(full["masks"][b, k], mask), (b, k)
        assert full["clicks"][b] == clicks, b
        assert np.array_equal(full["ious"][b], np.array(curve)), b       # bit for bit
        moved += curve[-1] != curve[0]
    assert moved > 0                                                   # the clicks changed something
    assert sum(len(c) for c in full["clicks"]) > 0


def test_summary_matches_the_curves(setup):
    from gcn_grabcut.metrics import noc_summary
    pipe, imgs, gts, full = setup
    want = noc_summary(full["ious"], (0.85, 0.90), CLICKS)
    assert set(full["noc"]) == {0.85, 0.90}
    for t in (0.85, 0.90):
        assert np.array_equal(full["noc"][t], want["noc"][t]) and full["nof"][t] == want["nof"][t]
    assert np.array_equal(full["mean_iou"], full["ious"].mean(axis=0))


def test_stop_iou_gives_prefixes_of_the_full_run(setup):
    pipe, imgs, gts, full = setup
    ious = full["ious"]
    stop = float(np.median(ious[:, 1]))
    part = pipe.evaluate_clicks(imgs, gts, max_clicks=CLICKS, hint_radius=RADIUS, stop_iou=stop, return_masks=True)
    stopped_early = 0
    for b in range(B):
        hit = np.nonzero(ious[b] >= stop)[0]
        s = int(hit[0]) if hit.size else CLICKS                        # the round after which image b gets no clicks
        stopped_early += s < CLICKS
        assert np.array_equal(part["ious"][b, :s + 1], ious[b, :s + 1]), b
        assert (part["ious"][b, s:] == ious[b, s]).all(), b
        assert np.array_equal(part["masks"][b, :s + 1], full["masks"][b, :s + 1]), b
        assert (part["masks"][b, s:] == full["masks"][b, s]).all(), b
        assert part["clicks"][b] == full["clicks"][b][:len(part["clicks"][b])], b
        assert len(part["clicks"][b]) <= s                             # clicks only in rounds 1..s
    assert stopped_early > 0


def test_argument_checks(setup):
    pipe, imgs, gts, full = setup
    with pytest.raises(ValueError):
        pipe.evaluate_clicks(imgs[:2], gts[:1])
    with pytest.raises(ValueError):
        pipe.evaluate_clicks(imgs[:1], [gts[0][:-1]])
    with pytest.raises(ValueError):
        pipe.evaluate_clicks(imgs[:1], gts[:1], iters_per_click=0)
