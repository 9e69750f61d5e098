"""The BFS relabel visit against the sweep visit, both as numpy restatements (relabel_visit_model.py): equal labels, equal nbm.

A tile is a 34x34 label window (tile + halo ring) and 32x32 arc bytes.  The BFS visit must either produce exactly what the
sweeps produce or hand the tile to them (start label below the BFS label, a labelled pixel the BFS does not reach, more
than LEVEL_CAP levels); the cases say which of the two each family has to take.
"""
import numpy as np
import pytest

import relabel_visit_model as M

DINF, T = M.DINF, M.T


def random_arcs(rng, density, h=T, w=T):
    """Arc bytes of an h x w image corner inside the tile: no arc leaves the image (the tile's halo counts as image where
    halo_in says so, below), pixels outside carry no arcs."""
    a = np.zeros((T, T), dtype=np.uint8)
    bits = rng.random((T, T, 8)) < density
    for d in range(8):
        a |= (bits[:, :, d].astype(np.uint8) << d)
    a[h:, :] = 0
    a[:, w:] = 0
    for d in range(8):                       # the image ends at row h / column w: arcs beyond it do not exist
        if M.DY[d] > 0 and h < T:
            a[h - 1, :] &= ~np.uint8(1 << d)
        if M.DX[d] > 0 and w < T:
            a[:, w - 1] &= ~np.uint8(1 << d)
    return a


def window(rng, inner, halo_lo=2, halo_hi=40, halo_p=0.5, h=T, w=T):
    win = np.full((T + 2, T + 2), DINF, dtype=np.int32)
    ring = rng.integers(halo_lo, halo_hi, size=(T + 2, T + 2)).astype(np.int32)
    ring[rng.random((T + 2, T + 2)) >= halo_p] = DINF
    win[:] = ring
    win[1:T + 1, 1:T + 1] = inner
    win[h + 1:, :] = DINF                    # below / right of the image
    win[:, w + 1:] = DINF
    return win


def fresh_inner(rng, p_sink):
    return np.where(rng.random((T, T)) < p_sink, 1, DINF).astype(np.int32)


def check(win, arcs, want_fallback=None):
    la, na, _ = M.visit_sweeps(win, arcs)
    lb, nb, fb = M.visit_bfs(win, arcs)
    assert np.array_equal(la, lb)
    assert na == nb
    if want_fallback is not None:
        assert fb == want_fallback
    return la, na


def test_bit_transpose():
    rng = np.random.default_rng(0)
    for _ in range(50):
        x = int(rng.integers(0, 1 << 63)) | (int(rng.integers(0, 2)) << 63)
        t = M.bit_transpose8(x)
        for i in range(8):
            for j in range(8):
                assert (x >> (8 * i + j)) & 1 == (t >> (8 * j + i)) & 1
        assert M.bit_transpose8(t) == x


def test_arc_rows():
    rng = np.random.default_rng(1)
    arcs = random_arcs(rng, 0.5)
    A = M.arc_rows(arcs)
    for d in range(8):
        for r in range(T):
            for x in range(T):
                assert (A[d][r] >> x) & 1 == (int(arcs[r, x]) >> d) & 1


@pytest.mark.parametrize("density", [0.05, 0.5, 0.95])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_tiles(density, seed):
    """Arbitrary start labels (1, finite, infinite): whichever way the visit goes, the result is the sweeps'."""
    rng = np.random.default_rng(100 * seed + int(density * 100))
    arcs = random_arcs(rng, density)
    inner = rng.integers(1, 30, size=(T, T)).astype(np.int32)
    inner[rng.random((T, T)) < 0.5] = DINF
    check(window(rng, inner), arcs)


@pytest.mark.parametrize("density", [0.05, 0.5, 0.95])
@pytest.mark.parametrize("p_sink", [0.002, 0.05])
def test_fresh_tiles(density, p_sink):
    """Labels 1 or infinity, as the start of a global relabel leaves them: the BFS itself has to give the result."""
    rng = np.random.default_rng(int(1000 * p_sink) + int(density * 100))
    arcs = random_arcs(rng, density)
    check(window(rng, fresh_inner(rng, p_sink)), arcs, want_fallback=False)


@pytest.mark.parametrize("density", [0.3, 0.95])
def test_revisit_lowered_halo(density):
    rng = np.random.default_rng(7 + int(density * 100))
    arcs = random_arcs(rng, density)
    win = window(rng, fresh_inner(rng, 0.01), halo_lo=30, halo_hi=60, halo_p=0.3)
    la, _ = check(win, arcs, want_fallback=False)
    for step in range(3):                    # the neighbours fell: a few halo labels are lower, the tile starts from its last result
        win[1:T + 1, 1:T + 1] = la
        ring = np.ones_like(win, dtype=bool)
        ring[1:T + 1, 1:T + 1] = False
        pick = ring & (rng.random(win.shape) < 0.1)
        win[pick] = rng.integers(2, 25 - 5 * step, size=int(pick.sum()))
        la, _ = check(win, arcs, want_fallback=False)
    win[1:T + 1, 1:T + 1] = la
    la2, nbm = check(win, arcs, want_fallback=False)
    assert nbm == 0 and np.array_equal(la, la2)          # a visit at the fixpoint changes nothing


def test_no_source():
    rng = np.random.default_rng(3)
    arcs = random_arcs(rng, 0.5)
    win = np.full((T + 2, T + 2), DINF, dtype=np.int32)
    la, nbm = check(win, arcs, want_fallback=False)
    assert nbm == 0 and (la == DINF).all()
    win[1:T + 1, 1:T + 1] = 7               # labelled pixels that nothing reaches: the sweeps' business
    win[5, 5] = DINF
    check(win, arcs, want_fallback=True)


def test_all_sink():
    rng = np.random.default_rng(4)
    arcs = random_arcs(rng, 0.5)
    win = window(rng, np.ones((T, T), dtype=np.int32))
    la, nbm = check(win, arcs, want_fallback=False)
    assert nbm == 0 and (la == 1).all()


@pytest.mark.parametrize("h,w", [(32, 12), (13, 32), (1, 1), (31, 17), (12, 31)])
def test_image_border(h, w):
    rng = np.random.default_rng(h * 40 + w)
    arcs = random_arcs(rng, 0.6, h, w)
    win = window(rng, fresh_inner(rng, 0.02), h=h, w=w)
    win[1:T + 1, 1:T + 1][h:, :] = DINF
    win[1:T + 1, 1:T + 1][:, w:] = DINF
    la, _ = check(win, arcs, want_fallback=False)
    assert (la[h:, :] == DINF).all() and (la[:, w:] == DINF).all()


def test_start_below_bfs_falls_back():
    """A pixel that starts below its BFS label carries its own label on: only the sweeps do that."""
    arcs = np.full((T, T), 0xFF, dtype=np.uint8)
    arcs[0, :] &= ~np.uint8(0b01010100); arcs[T - 1, :] &= ~np.uint8(0b10101000)
    arcs[:, 0] &= ~np.uint8(0b10010001); arcs[:, T - 1] &= ~np.uint8(0b01100010)
    win = np.full((T + 2, T + 2), DINF, dtype=np.int32)
    win[1, 1] = 1
    win[21, 21] = 3                          # its BFS label is 21
    la, _ = check(win, arcs, want_fallback=True)
    assert la[20, 20] == 3 and la[20, 24] == 7 and la[10, 10] == 11


def spiral():
    path, y, x = [(0, 0)], 0, 0
    top, bot, lef, rig = 0, T - 1, 0, T - 1
    while True:
        n = len(path)
        while x < rig: x += 1; path.append((y, x))
        rig -= 2
        while y < bot: y += 1; path.append((y, x))
        bot -= 2
        while x > lef: x -= 1; path.append((y, x))
        lef += 2
        top += 2
        while y > top: y -= 1; path.append((y, x))
        if len(path) == n:
            return path


def test_spiral_corridor_hits_the_cap():
    path = spiral()
    assert len(path) > 4 * M.LEVEL_CAP and len(set(path)) == len(path)
    arcs = np.zeros((T, T), dtype=np.uint8)
    for (y0, x0), (y1, x1) in zip(path[:-1], path[1:]):
        d = [k for k in range(4) if (M.DX[k], M.DY[k]) == (x1 - x0, y1 - y0)][0]
        arcs[y0, x0] |= 1 << d
        arcs[y1, x1] |= 1 << (d ^ 1)
    win = np.full((T + 2, T + 2), DINF, dtype=np.int32)
    win[1, 1] = 1
    ok, _, _, levels = M.bfs_levels(win, arcs)
    assert not ok and levels == M.LEVEL_CAP
    la, nbm = check(win, arcs, want_fallback=True)
    for i, (y, x) in enumerate(path):
        assert la[y, x] == i + 1
