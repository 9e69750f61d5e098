"""ggc_next_click on the MI355X against a NumPy / scipy restatement of the NoC click rule (include/ggc.h, C0): row, col,
label and d2 must agree exactly, image by image and for a mixed batch."""
import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- restatement of ggc_next_click

def region_d2(region):
    """Squared distance of every pixel of `region` to the nearest pixel outside it, the image padded by one pixel of
    zeros; 0 outside the region."""
    if not region.any():
        return np.zeros(region.shape, np.int64)
    d = ndimage.distance_transform_edt(np.pad(region, 1))[1:-1, 1:-1]
    return np.rint(d * d).astype(np.int64)


def next_click(pred, gt):
    """-> (row, col, label, d2): label 1 = foreground click in fn, 0 = background click in fp; (-1, -1, -1, 0) when
    pred == gt.  A tie of the two maxima goes to the background click; the first raster index wins among equal d2."""
    pred, gt = np.asarray(pred) != 0, np.asarray(gt) != 0
    d_fn, d_fp = region_d2(gt & ~pred), region_d2(~gt & pred)
    m_fn, m_fp = int(d_fn.max()), int(d_fp.max())
    if m_fn == 0 and m_fp == 0:
        return (-1, -1, -1, 0)
    d, label = (d_fn, 1) if m_fn > m_fp else (d_fp, 0)
    r, c = np.unravel_index(int(np.argmax(d)), d.shape)             # argmax: the first of equal maxima in raster order
    return (int(r), int(c), label, int(d[r, c]))


# ---------------------------------------------------------------- inputs

def blobs(rng, h, w, n):
    """(H,W) bool: a union of n random ellipses (some may leave the frame)."""
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for _ in range(n):
        cy, cx = rng.uniform(-0.1, 1.1) * h, rng.uniform(-0.1, 1.1) * w
        ry, rx = rng.uniform(0.05, 0.4) * h + 0.5, rng.uniform(0.05, 0.4) * w + 0.5
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return m


def blob_case(seed, h, w):
    """A ground truth and a prediction that misses some of it and adds some: realistic fn and fp regions."""
    rng = np.random.default_rng(seed)
    gt = blobs(rng, h, w, int(rng.integers(1, 4)))
    pred = (gt & ~blobs(rng, h, w, int(rng.integers(1, 3)))) | blobs(rng, h, w, int(rng.integers(1, 3)))
    if h * w > 1 and (pred == gt).all():
        pred[0, 0] = ~pred[0, 0]
    return pred.astype(np.uint8), gt.astype(np.uint8)


def run(preds, gts):
    from gcn_grabcut._engine import get_engine
    eng = get_engine("cuda")
    p = eng.to_device(np.ascontiguousarray(np.stack(preds), np.uint8))
    g = eng.to_device(np.ascontiguousarray(np.stack(gts), np.uint8))
    return [tuple(int(v) for v in row) for row in eng.next_click(p, g).cpu().numpy()]


def check(preds, gts):
    got = run(preds, gts)
    for i, (p, g) in enumerate(zip(preds, gts)):
        assert got[i] == next_click(p, g), (i, p.shape)
    return got


# ---------------------------------------------------------------- cases

@pytest.mark.parametrize("h,w", [(1, 1), (1, 57), (61, 1), (37, 53), (300, 400)])
def test_random_blobs(h, w):
    cases = [blob_case(1000 * h + w + s, h, w) for s in range(4)]
    if h * w == 1:
        cases = [(np.ones((1, 1), np.uint8), np.zeros((1, 1), np.uint8)), (np.zeros((1, 1), np.uint8), np.ones((1, 1), np.uint8)),
                 (np.ones((1, 1), np.uint8), np.ones((1, 1), np.uint8))]
    got = check([p for p, _ in cases], [g for _, g in cases])
    if h * w > 1:
        assert any(c[0] >= 0 for c in got)


def test_no_error_gives_no_click():
    rng = np.random.default_rng(2)
    gt = blobs(rng, 40, 50, 2).astype(np.uint8)
    assert check([gt, np.zeros_like(gt)], [gt, np.zeros_like(gt)]) == [(-1, -1, -1, 0)] * 2


def test_every_pixel_an_error():
    h, w = 29, 44
    ones, zeros = np.ones((h, w), np.uint8), np.zeros((h, w), np.uint8)
    got = check([zeros, ones], [ones, zeros])
    assert got[0][2] == 1 and got[1][2] == 0                         # all fn: a foreground click; all fp: background
    assert got[0][3] == 15 * 15                                      # the centre row is 15 from the padding


def test_errors_touching_the_border():
    h, w = 31, 47
    gt = np.zeros((h, w), np.uint8)
    gt[:, :9] = 1                                                    # a band along the left edge, missed
    gt[-5:, 20:] = 1                                                 # and one along the bottom right
    pred = np.zeros_like(gt)
    pred[:6, 30:] = 1                                                # a false positive in the top right corner
    got = check([pred], [gt])
    assert got[0][2] == 1


def test_fp_only():
    h, w = 45, 60
    gt = np.zeros((h, w), np.uint8)
    gt[10:30, 10:40] = 1
    pred = gt.copy()
    pred[5:9, 45:58] = 1
    pred[33:44, 2:6] = 1
    got = check([pred], [gt])
    assert got[0][2] == 0


def test_tie_goes_to_the_background_click():
    gt = np.zeros((20, 40), np.uint8)
    pred = np.zeros_like(gt)
    gt[5:12, 25:32] = 1                                              # a 7x7 fn square on the right
    pred[5:12, 4:11] = 1                                             # the same square as fp on the left
    r = next_click(pred, gt)
    d_fn, d_fp = region_d2(gt & ~pred != 0), region_d2(~gt & pred != 0)
    assert d_fn.max() == d_fp.max() == 16
    got = check([pred], [gt])
    assert got[0] == r and r[2] == 0 and r[1] < 20


def test_many_equal_maxima_first_raster_index_wins():
    gt = np.zeros((23, 70), np.uint8)
    for c in range(3, 66, 7):                                        # ten 3x3 fn squares, each d2 = 4 at its centre
        for r in (4, 15):
            gt[r:r + 3, c:c + 3] = 1
    pred = np.zeros_like(gt)
    got = check([pred], [gt])
    assert got[0] == (5, 4, 1, 4)


def test_gt_as_0_255():
    cases = [blob_case(77 + s, 50, 64) for s in range(3)]
    preds = [p for p, _ in cases]
    got01 = run(preds, [g for _, g in cases])
    got255 = check(preds, [g * 255 for _, g in cases])
    assert got01 == got255
    got_pred255 = run([p * 255 for p in preds], [g * 255 for _, g in cases])
    assert got_pred255 == got01


def test_mixed_batch_equals_one_at_a_time():
    h, w = 48, 66
    cases = [blob_case(500 + s, h, w) for s in range(5)]
    gt = cases[0][1]
    cases.append((gt.copy(), gt.copy()))                             # no click
    cases.append((np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)))
    pred = gt.copy()
    pred[0:4, 0:4] = 1 - pred[0:4, 0:4]
    cases.append((pred, gt))
    preds, gts = [p for p, _ in cases], [g for _, g in cases]
    batched = check(preds, gts)
    assert batched == [run([p], [g])[0] for p, g in zip(preds, gts)]
    assert batched == run(preds, gts)                                # repeatable


def test_argument_checks():
    from gcn_grabcut import _native
    from gcn_grabcut._engine import get_engine
    eng = get_engine("cuda")
    m = torch.zeros(0, 5, 7, dtype=torch.uint8, device=eng.device)
    assert eng.next_click(m, m).shape == (0, 4)                      # B == 0: a no-op
    wide = torch.zeros(1, 2, 9000, dtype=torch.uint8, device=eng.device)
    with pytest.raises(_native.GGCError, match="INVALID_ARG"):
        eng.next_click(wide, wide)
    out = torch.empty(1, 4, dtype=torch.int32, device=eng.device)
    with pytest.raises(_native.GGCError, match="INVALID_ARG"):
        eng.ctx.call("ggc_next_click", eng._stream(), 1, 0, 5, wide.data_ptr(), wide.data_ptr(), out.data_ptr())
