"""The magic wand on the MI355X: ggc_wand_select through the C ABI against tests/wand_ref.py (a queue flood fill), bit for
bit on mask, select and counts.  The shapes put waves of the labelling kernels across rows, seed planes and images; the
patterns are the ones a run-based union-find can get wrong."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import wand_cases as cases
import wand_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
POISON_SELECT, POISON_COUNT = 7, -5


@pytest.fixture(scope="module")
def eng():
    from gcn_grabcut._engine import get_engine
    return get_engine("cuda")


def label_mask(b, h, w, seed=1):
    """All four GrabCut labels, so that an untouched pixel shows."""
    return np.random.default_rng(seed).integers(0, 4, (b, h, w)).astype(np.uint8)


def call(eng, imgs, seeds, ptr, tol, conn, sample, mask=None, select=True, counts=True):
    """One ggc_wand_select call on poisoned outputs -> (mask, select, counts) on the host, None for an absent one."""
    imgs = np.ascontiguousarray(imgs, np.uint8)
    b, h, w, _ = imgs.shape
    d_img = eng.to_device(imgs)
    d_seeds = eng.to_device(np.ascontiguousarray(seeds, np.int32).reshape(-1, 3))
    d_ptr = eng.to_device(np.ascontiguousarray(ptr, np.int32))
    d_mask = None if mask is None else eng.to_device(np.ascontiguousarray(mask, np.uint8))
    d_sel = torch.full((b, h, w), POISON_SELECT, dtype=torch.uint8, device="cuda") if select else None
    d_cnt = torch.full((b, 2), POISON_COUNT, dtype=torch.int32, device="cuda") if counts else None
    eng.ctx.call("ggc_wand_select", eng._stream(), b, h, w, d_img.data_ptr(), d_seeds.data_ptr() if len(seeds) else None,
                 d_ptr.data_ptr(), int(tol), int(conn), int(sample), None if d_mask is None else d_mask.data_ptr(),
                 None if d_sel is None else d_sel.data_ptr(), None if d_cnt is None else d_cnt.data_ptr())
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (d_mask, d_sel, d_cnt))


def check(eng, imgs, per_image, tol, conn, sample, what=""):
    """All three outputs of one call against the reference; the mask starts with all four labels."""
    imgs = np.asarray(imgs)
    seeds, ptr = cases.pack(per_image)
    mask = label_mask(*imgs.shape[:3])
    want = ref.wand_batch(imgs, seeds, ptr, tol, conn, sample, mask)
    got = call(eng, imgs, seeds, ptr, tol, conn, sample, mask)
    for name, g, w in zip(("mask", "select", "counts"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, imgs.shape, tol, conn, sample)
    return want


def corner_seeds(h, w):
    """Foreground at the first pixel, background at the last, foreground in the middle, background on the top edge."""
    return [(0, 0, 1), (h - 1, w - 1, 0), (h // 2, w // 2, 1), (0, w // 2, 0)]


@pytest.mark.parametrize("h", [1, 2, 7])
@pytest.mark.parametrize("w", [1, 63, 64, 65, 129])
def test_thin_and_wave_sized_shapes(eng, h, w):
    rng = np.random.default_rng(100 * h + w)
    plane = cases.blocky(rng, h, w, 2, 3)
    for noisy in (False, True):
        img = cases.to_image(plane, noisy, seed=w)
        for conn in (4, 8, 0):
            for sample in (1, 3, 5):
                check(eng, img[None], [corner_seeds(h, w)], cases.NOISE if noisy else 0, conn, sample, f"noisy={noisy}")


def test_one_pixel(eng):
    img = np.array([[[9, 8, 7]]], np.uint8)
    for conn in (4, 8, 0):
        want = check(eng, img[None], [[(0, 0, 1)]], 0, conn, 5)
        assert want[1][0, 0, 0] == 255 and want[2].tolist() == [[1, 0]]
        check(eng, img[None], [[(0, 0, 1), (0, 0, 0)]], 0, conn, 1)


def test_waves_straddle_seed_planes(eng):
    """5 x 13: P = 65 is no multiple of 64, so with two and three seeds a wave holds the end of one plane and the start
    of the next."""
    rng = np.random.default_rng(5)
    for plane in (cases.blocky(rng, 5, 13, 2, 2), np.ones((5, 13), np.uint8), cases.comb(5, 13)):
        img = cases.to_image(plane)
        for conn in (4, 8, 0):
            check(eng, img[None], [[(0, 0, 1), (4, 12, 0)]], 0, conn, 1)
            check(eng, img[None], [[(4, 12, 1), (2, 6, 0), (0, 0, 1)]], 0, conn, 1)
            check(eng, img[None], [[(4, 12, 1), (2, 6, 0), (0, 0, 1)]], 255, conn, 3)


def test_batch_with_an_empty_image_and_an_outside_seed(eng):
    rng = np.random.default_rng(6)
    imgs = np.stack([cases.to_image(cases.blocky(rng, 7, 65, 3, 3)) for _ in range(3)])
    for conn in (4, 8, 0):
        want = check(eng, imgs, [[(3, 3, 1), (6, 64, 0)], [], [(7, 0, 1)]], 0, conn, 1)
        assert want[2][1].tolist() == [0, 0] and want[2][2].tolist() == [0, 0] and not want[1][1:].any()
        check(eng, imgs, [[(-1, 0, 1)], [], [(0, 65, 0)]], 0, conn, 1)           # every seed outside: select and counts are zeros


PATTERNS = {
    "diagonal_down": lambda: (cases.diagonal(17, 17, True), [(0, 0, 1), (16, 0, 0)]),
    "diagonal_up": lambda: (cases.diagonal(17, 17, False), [(0, 16, 1), (0, 0, 0)]),
    "staircase_down": lambda: (cases.staircase(23, 70, True), [(0, 0, 1), (22, 0, 0)]),
    "staircase_up": lambda: (cases.staircase(23, 70, False), [(0, 69, 1), (22, 69, 0)]),
    "comb": lambda: (cases.comb(9, 67), [(8, 0, 1), (8, 1, 0), (8, 66, 1)]),
    "spiral": lambda: (cases.spiral(33), [(0, 0, 1), (1, 0, 0)]),
    "ring": lambda: (cases.ring(12, 66), [(0, 0, 1), (1, 1, 0)]),
    "flat": lambda: (np.zeros((6, 130), np.uint8), [(3, 64, 1)]),
}


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_patterns_at_every_connectivity(eng, name):
    plane, seeds = PATTERNS[name]()
    for noisy in (False, True):
        img = cases.to_image(plane, noisy, seed=3)
        for conn in (4, 8, 0):
            check(eng, img[None], [seeds], cases.NOISE if noisy else 0, conn, 1, name)


def test_patterns_are_what_they_claim():
    """The shapes do what they were chosen for, by the reference alone."""
    d = cases.to_image(cases.diagonal(17, 17))
    assert ref.selection(d, 0, 0, 0, 4, 1).sum() == 1 and ref.selection(d, 0, 0, 0, 8, 1).sum() == 17
    s = cases.spiral(33)
    assert s.sum() > 500 and ref.selection(cases.to_image(s), 0, 0, 0, 4, 1).sum() == s.sum()
    r = cases.to_image(cases.ring(12, 66))
    assert not ref.selection(r, 0, 0, 0, 8, 1)[5, 30] and ref.selection(r, 0, 0, 0, 0, 1)[5, 30]


def test_runs_across_flat_index_64(eng):
    """W = 65: a run crosses flat index 64 at x = 64 and must stay one run.  W = 64: flat index 64 is x = 0 of row 1, and
    the end of row 0 must not join it."""
    p65 = np.zeros((3, 65), np.uint8)
    p65[0, 58:] = 1
    p64 = np.zeros((3, 64), np.uint8)
    p64[0, 58:] = 1
    p64[1, :5] = 1
    p128 = np.zeros((2, 128), np.uint8)
    p128[0, 60:70] = 1
    p128[1, 120:] = 1
    for plane, seeds in ((p65, [(0, 58, 1), (0, 64, 0)]), (p64, [(0, 63, 1), (1, 0, 0), (0, 60, 1)]), (p128, [(0, 60, 1), (1, 127, 0)])):
        img = cases.to_image(plane)
        for conn in (4, 8):
            want = check(eng, img[None], [seeds], 0, conn, 1)
            if plane is p64:
                assert want[2].tolist() == [[6, 5]]                               # the two runs stay apart


@pytest.mark.parametrize("tol", [0, 1, 254, 255])
def test_tolerances(eng, tol):
    rng = np.random.default_rng(tol)
    img = np.ascontiguousarray(rng.choice(np.array([0, 1, 2, 128, 253, 254, 255], np.uint8), (9, 66, 3)))
    for conn in (4, 8, 0):
        for sample in (1, 3):
            check(eng, img[None], [[(0, 0, 1), (8, 65, 0), (4, 30, 1)]], tol, conn, sample)


@pytest.mark.parametrize("sample", [1, 3, 5])
def test_sample_windows_at_corners_and_edges(eng, sample):
    rng = np.random.default_rng(sample)
    img = cases.quantised(rng, 8, 67, 4)
    h, w = img.shape[:2]
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, 33), (h - 1, 33), (4, 0), (4, w - 1), (1, 1), (4, 40)]
    for conn in (4, 8, 0):
        for tol in (40, 100):
            check(eng, img[None], [[(r, c, (i + 1) % 2) for i, (r, c) in enumerate(spots)]], tol, conn, sample)


def test_the_last_seed_wins(eng):
    img = cases.to_image(np.zeros((6, 70), np.uint8))
    for conn in (4, 8, 0):
        a = check(eng, img[None], [[(0, 0, 1), (5, 69, 0)]], 0, conn, 1)
        b = check(eng, img[None], [[(0, 0, 0), (5, 69, 1)]], 0, conn, 1)
        assert a[2].tolist() == [[0, 420]] and not a[1].any() and b[2].tolist() == [[420, 0]] and (b[1] == 255).all()
    plane = np.zeros((6, 70), np.uint8)
    plane[:, 35:] = 2
    img = cases.to_image(plane)
    for conn in (4, 8, 0):                                                        # tolerance 255 covers both halves, 0 one
        check(eng, img[None], [[(0, 0, 1), (0, 69, 0)]], 255, conn, 1)
        c = call(eng, img[None], *cases.pack([[(0, 0, 1), (0, 69, 0)]]), 0, conn, 1)
        assert c[2].tolist() == [[210, 210]]


def test_each_output_may_be_absent(eng):
    rng = np.random.default_rng(8)
    imgs = np.stack([cases.to_image(cases.blocky(rng, 9, 65, 3, 3)) for _ in range(2)])
    seeds, ptr = cases.pack([[(0, 0, 1), (8, 64, 0)], [(4, 4, 0), (4, 40, 1)]])
    mask = label_mask(2, 9, 65)
    for conn in (8, 0):
        want = ref.wand_batch(imgs, seeds, ptr, 0, conn, 1, mask)
        for keep in ((1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            got = call(eng, imgs, seeds, ptr, 0, conn, 1, mask if keep[0] else None, bool(keep[1]), bool(keep[2]))
            for k, g, w in zip(keep, got, want):
                assert (g is None and not k) or np.array_equal(g, w), (conn, keep)


def test_every_image_equals_its_single_call(eng):
    rng = np.random.default_rng(9)
    imgs = np.stack([cases.quantised(rng, 11, 65, 3) for _ in range(4)])
    per_image = [[(0, 0, 1), (10, 64, 0), (5, 5, 1)], [], [(3, 3, 0)], [(2, 60, 1), (2, 61, 0), (20, 0, 1), (9, 1, 1)]]
    for conn in (4, 8, 0):
        whole = check(eng, imgs, per_image, 90, conn, 3)
        mask = label_mask(4, 11, 65)
        for b in range(4):
            if not per_image[b]:
                continue                                                          # without a seed the call is a no-op
            seeds, ptr = cases.pack([per_image[b]])
            one = call(eng, imgs[b:b + 1], seeds, ptr, 90, conn, 3, mask[b:b + 1])
            for g, w in zip(one, whole):
                assert np.array_equal(g[0], w[b]), (conn, b)


PASS_SCRIPT = """
import sys
import numpy as np, torch
sys.path[:0] = [r'{root}', r'{root}/src', r'{root}/tests']
import wand_cases as cases
from test_wand_gpu import call, pass_case
from gcn_grabcut._engine import get_engine
eng = get_engine('cuda')
img, seeds, ptr, mask = pass_case()
for conn in (4, 8, 0):
    got = call(eng, img, seeds, ptr, 0, conn, 1, mask)
    print('RESULT', conn, ' '.join(g.tobytes().hex() for g in got))
"""


def pass_case():
    """Two images, the first with 5 overlapping seeds of mixed labels on 3 levels, the second with 2."""
    rng = np.random.default_rng(21)
    img = np.stack([cases.to_image(cases.blocky(rng, 40, 70, 3, 5)) for _ in range(2)])
    seeds, ptr = cases.pack([[(0, 0, 1), (39, 69, 0), (20, 35, 1), (0, 0, 0), (20, 36, 1)], [(5, 5, 0), (30, 60, 1)]])
    return img, seeds, ptr, label_mask(2, 40, 70)


def test_the_pass_size_changes_no_output(tmp_path):
    """GGC_WAND_SEEDS_PER_PASS is read once per process: one child per value, each under its own time limit; a child that
    fails or runs out of time ends the test."""
    img, seeds, ptr, mask = pass_case()
    want = {conn: ref.wand_batch(img, seeds, ptr, 0, conn, 1, mask) for conn in (4, 8, 0)}
    script = tmp_path / "passes.py"
    script.write_text(PASS_SCRIPT.format(root=ROOT))
    for per_pass in ("", "1", "2"):
        env = dict(os.environ)
        env.pop("GGC_WAND_SEEDS_PER_PASS", None)
        if per_pass:
            env["GGC_WAND_SEEDS_PER_PASS"] = per_pass
        r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (per_pass, r.stderr[-2000:])
        lines = [x.split() for x in r.stdout.splitlines() if x.startswith("RESULT")]
        assert [int(x[1]) for x in lines] == [4, 8, 0], (per_pass, r.stdout[-500:])
        for x in lines:
            assert x[2:] == [w.tobytes().hex() for w in want[int(x[1])]], (per_pass, x[1])


def test_refusals_leave_the_outputs_alone(eng):
    from gcn_grabcut._native import GGCError
    img = eng.to_device(np.zeros((2, 4, 4, 3), np.uint8))
    seeds = eng.to_device(np.array([[0, 0, 1], [1, 1, 0]], np.int32))
    ptr = eng.to_device(np.array([0, 1, 2], np.int32))
    bad0 = eng.to_device(np.array([1, 1, 2], np.int32))
    down = eng.to_device(np.array([0, 2, 1], np.int32))
    mask = torch.full((2, 4, 4), 3, dtype=torch.uint8, device="cuda")
    sel = torch.full((2, 4, 4), POISON_SELECT, dtype=torch.uint8, device="cuda")
    cnt = torch.full((2, 2), POISON_COUNT, dtype=torch.int32, device="cuda")
    ok = dict(b=2, h=4, w=4, bgr=img.data_ptr(), seeds=seeds.data_ptr(), ptr=ptr.data_ptr(), tol=10, conn=8, sample=1,
              mask=mask.data_ptr(), sel=sel.data_ptr(), cnt=cnt.data_ptr())

    def code(**change):
        a = dict(ok, **change)
        with pytest.raises(GGCError) as e:
            eng.ctx.call("ggc_wand_select", eng._stream(), a["b"], a["h"], a["w"], a["bgr"], a["seeds"], a["ptr"], a["tol"],
                         a["conn"], a["sample"], a["mask"], a["sel"], a["cnt"])
        message = eng.ctx.lib.ggc_last_error(eng.ctx.handle)
        assert message and len(message) > 0 and message.decode() in str(e.value)  # ggc_last_error is set
        return e.value.code

    for change in (dict(b=65536), dict(b=-1), dict(h=0), dict(w=0), dict(h=65536), dict(w=65536), dict(h=65535, w=65535)):
        assert code(**change) == -2, change                                       # GGC_E_SHAPE
    for change in (dict(tol=-1), dict(tol=256), dict(conn=1), dict(conn=6), dict(conn=-4), dict(sample=0), dict(sample=2),
                   dict(sample=7), dict(bgr=None), dict(ptr=None), dict(seeds=None), dict(ptr=bad0.data_ptr()),
                   dict(ptr=down.data_ptr()), dict(mask=None, sel=None, cnt=None)):
        assert code(**change) == -1, change                                       # GGC_E_INVALID_ARG
    torch.cuda.synchronize()
    assert (mask == 3).all() and (sel == POISON_SELECT).all() and (cnt == POISON_COUNT).all()


def test_no_ops_write_nothing(eng):
    img = np.zeros((2, 4, 4, 3), np.uint8)
    mask = np.full((2, 4, 4), 3, np.uint8)
    none = np.zeros((0, 3), np.int32)
    for conn in (4, 8, 0):
        got = call(eng, img, none, np.zeros(3, np.int32), 10, conn, 1, mask)      # seed_ptr[B] == 0
        assert (got[0] == 3).all() and (got[1] == POISON_SELECT).all() and (got[2] == POISON_COUNT).all()
    sel = torch.full((2, 4, 4), POISON_SELECT, dtype=torch.uint8, device="cuda")
    eng.ctx.call("ggc_wand_select", eng._stream(), 0, 4, 4, None, None, None, 10, 8, 1, None, sel.data_ptr(), None)   # B == 0
    torch.cuda.synchronize()
    assert (sel == POISON_SELECT).all()
