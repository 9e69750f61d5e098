"""numpy restatements of the two relabel tile visits of ggc_mf_sweep.h, on one tile.

Inputs of a visit, as the kernel has them in LDS after its load phase:
  win   int32 [34][34]  labels of the 32x32 tile (win[1:33, 1:33]) and of its halo ring; DINF outside the image
  arcs  uint8 [32][32]  bit dir = residual arc of the pixel towards dir (0 for a pixel outside the image)
Output of a visit: (labels int32 [32][32], nbm) — nbm is the 9-bit mask of the neighbour tiles whose halo changed,
bit (dy + 1) * 3 + (dx + 1), with bit 4 when the sweeps stopped short of the fixpoint.

visit_sweeps  mf_relax_visit: V and H sweeps (a lane owns 16 pixels of a column / of a row, reads its window once and
              runs a forward and a backward pass over its pixels in registers), until a sweep changes nothing.
visit_bfs     mf_relax_visit_bfs: arc bit rows by an 8x8 bit transpose, a level-synchronous multi-source BFS on bit rows
              (level indices in bit planes, level values in a table), and the sweeps as the fallback.
"""
from __future__ import annotations

import numpy as np

DINF = 1 << 29
T = 32
SWEEP_CAP = 4 * T          # the sweep loop of mf_relax_visit
LEVEL_CAP = 96             # MF_BFS_CAP of ggc_mf_sweep.h
# directions: 0 left, 1 right, 2 up, 3 down, 4 up-left, 5 down-right, 6 up-right, 7 down-left
DX = (-1, 1, 0, 0, -1, 1, 1, -1)
DY = (0, 0, -1, 1, -1, 1, -1, 1)
U32 = 0xFFFFFFFF


def _gated(v, arcs, bit):
    """v where the arc exists, >= DINF otherwise (the kernel ORs the infinite bit in)."""
    return np.where((arcs >> bit) & 1, v, v | DINF)


def _relax5(c, arcs, bits, vals):
    nd = _gated(vals[0], arcs, bits[0])
    for b, v in zip(bits[1:], vals[1:]):
        nd = np.minimum(nd, _gated(v, arcs, b))
    return np.minimum(c, nd + 1)


def _sweep_v(win, arcs):
    """relax_sweep_v: every lane from one snapshot; only its own column is updated as it walks."""
    snap = win.copy()
    col = snap[:, 1:33].copy()                     # col[a][lx]: the lane's own column, rows 0..33 of the window
    left, right = snap[:, 0:32], snap[:, 2:34]     # the neighbour columns stay as read
    for h in (0, 1):
        seg = col.copy()                           # a lane sees the other half's pixels as read
        for r in range(16):
            a = 16 * h + r + 1
            seg[a] = _relax5(seg[a], arcs[a - 1], (0, 1, 2, 4, 6), (left[a], right[a], seg[a - 1], left[a - 1], right[a - 1]))
        for r in range(15, -1, -1):
            a = 16 * h + r + 1
            seg[a] = _relax5(seg[a], arcs[a - 1], (0, 1, 3, 5, 7), (left[a], right[a], seg[a + 1], right[a + 1], left[a + 1]))
        win[16 * h + 1:16 * h + 17, 1:33] = seg[16 * h + 1:16 * h + 17]
    return not np.array_equal(win, snap)


def _sweep_h(win, arcs):
    snap = win.copy()
    row = snap[1:33, :].copy()                     # row[ly][c]
    up, down = snap[0:32, :], snap[2:34, :]
    for h in (0, 1):
        seg = row.copy()
        for k in range(16):
            c = 16 * h + k + 1
            seg[:, c] = _relax5(seg[:, c], arcs[:, c - 1], (2, 3, 0, 4, 7), (up[:, c], down[:, c], seg[:, c - 1], up[:, c - 1], down[:, c - 1]))
        for k in range(15, -1, -1):
            c = 16 * h + k + 1
            seg[:, c] = _relax5(seg[:, c], arcs[:, c - 1], (2, 3, 1, 6, 5), (up[:, c], down[:, c], seg[:, c + 1], up[:, c + 1], down[:, c + 1]))
        win[1:33, 16 * h + 1:16 * h + 17] = seg[:, 16 * h + 1:16 * h + 17]
    return not np.array_equal(win, snap)


def _nbm(old, new, settled):
    ch = new != old
    U, D, Lf, Rt = ch[0].any(), ch[T - 1].any(), ch[:, 0].any(), ch[:, T - 1].any()
    nbm = 0 if settled else 1 << 4
    nbm |= int(ch[0, 0]) | int(U) << 1 | int(ch[0, T - 1]) << 2 | int(Lf) << 3 | int(Rt) << 5
    nbm |= int(ch[T - 1, 0]) << 6 | int(D) << 7 | int(ch[T - 1, T - 1]) << 8
    return nbm


def visit_sweeps(win, arcs):
    win = np.array(win, dtype=np.int64)
    arcs = np.asarray(arcs).astype(np.int64)
    old = win[1:33, 1:33].copy()
    settled = False
    n = 0
    for it in range(SWEEP_CAP):
        ch = _sweep_h(win, arcs) if it & 1 else _sweep_v(win, arcs)
        n += 1
        if not ch:
            settled = True
            break
    new = win[1:33, 1:33]
    return new.astype(np.int32), _nbm(old, new, settled), n


# ---- the BFS visit ---------------------------------------------------------------------------------------------------
def bit_transpose8(x: int) -> int:
    """8x8 bit transpose of a 64-bit word: bit 8 i + j <-> bit 8 j + i."""
    M = 0xFFFFFFFFFFFFFFFF
    t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AA
    x = (x ^ t ^ (t << 7)) & M
    t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCC
    x = (x ^ t ^ (t << 14)) & M
    t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0
    x = (x ^ t ^ (t << 28)) & M
    return x


def arc_rows(arcs):
    """A[dir][r]: bit x set when pixel (r, x) has a residual arc towards dir — from the INVERTED mask bytes, as the kernel."""
    inv = (~np.asarray(arcs).astype(np.int64)) & 0xFF
    A = [[0] * T for _ in range(8)]
    for r in range(T):
        for g in range(4):
            x = 0
            for i in range(8):
                x |= int(inv[r, 8 * g + i]) << (8 * i)
            x = bit_transpose8(x)
            for d in range(8):
                A[d][r] |= ((x >> (8 * d)) & 0xFF) << (8 * g)
        for d in range(8):
            A[d][r] = ~A[d][r] & U32
    return A


def _entry(vals_bits):
    e = DINF
    for v, open_ in vals_bits:
        if open_:
            e = min(e, int(v))
    return min(e + 1, DINF)


def bfs_levels(win, arcs):
    """The level loop.  Returns (ok, label [32][32] with DINF where not reached, reached mask, levels processed)."""
    win = np.asarray(win).astype(np.int64)
    A = arc_rows(arcs)
    bit = lambda d, r, x: (A[d][r] >> x) & 1
    one = [0] * T
    for r in range(T):
        for x in range(T):
            if win[r + 1, x + 1] == 1:
                one[r] |= 1 << x
    eL = [_entry(((win[r, 0], bit(4, r, 0)), (win[r + 1, 0], bit(0, r, 0)), (win[r + 2, 0], bit(7, r, 0)))) for r in range(T)]
    eR = [_entry(((win[r, 33], bit(6, r, 31)), (win[r + 1, 33], bit(1, r, 31)), (win[r + 2, 33], bit(5, r, 31)))) for r in range(T)]
    eT = [_entry(((win[0, x], bit(4, 0, x)), (win[0, x + 1], bit(2, 0, x)), (win[0, x + 2], bit(6, 0, x)))) for x in range(T)]
    eB = [_entry(((win[33, x], bit(7, 31, x)), (win[33, x + 1], bit(3, 31, x)), (win[33, x + 2], bit(5, 31, x)))) for x in range(T)]
    done = [0] * T
    front = [0] * T
    planes = [[0] * T for _ in range(7)]
    lv = [0] * LEVEL_CAP
    def next_level():
        """The lowest entry level still pending, DINF if none."""
        cand = DINF
        for r in range(T):
            if one[r] & ~done[r]:
                cand = min(cand, 1)
            if not done[r] & 1:
                cand = min(cand, eL[r])
            if not (done[r] >> 31) & 1:
                cand = min(cand, eR[r])
        for x in range(T):
            if not (done[0] >> x) & 1:
                cand = min(cand, eT[x])
            if not (done[31] >> x) & 1:
                cand = min(cand, eB[x])
        return cand

    L = next_level()
    finished = L >= DINF
    k = 0
    while k < LEVEL_CAP and not finished:
        lv[k] = L
        top = sum(1 << x for x in range(T) if eT[x] == L)
        bot = sum(1 << x for x in range(T) if eB[x] == L)
        new = [0] * T
        for r in range(T):
            fu = front[r - 1] if r > 0 else 0
            fd = front[r + 1] if r < T - 1 else 0
            f = front[r]
            reach = (A[0][r] & (f << 1)) | (A[1][r] & (f >> 1)) | (A[2][r] & fu) | (A[3][r] & fd) \
                | (A[4][r] & (fu << 1)) | (A[5][r] & (fd >> 1)) | (A[6][r] & (fu >> 1)) | (A[7][r] & (fd << 1))
            own = (1 if eL[r] == L else 0) | ((1 << 31) if eR[r] == L else 0)
            if r == 0:
                own |= top
            if r == T - 1:
                own |= bot
            if L == 1:
                own |= one[r]
            new[r] = (reach | own) & ~done[r] & U32
        for r in range(T):
            done[r] |= new[r]
            for j in range(7):
                if (k >> j) & 1:
                    planes[j][r] |= new[r]
        front = new
        k += 1
        if any(front):
            L += 1
        else:                                   # the front ran dry
            L = next_level()
            finished = L >= DINF
    if not finished:
        return False, None, None, LEVEL_CAP
    lab = np.full((T, T), DINF, dtype=np.int64)
    reached = np.zeros((T, T), dtype=bool)
    for r in range(T):
        for g in range(4):
            x = 0
            for j in range(7):
                x |= ((planes[j][r] >> (8 * g)) & 0xFF) << (8 * j)
            x = bit_transpose8(x)
            for i in range(8):
                c = 8 * g + i
                if (done[r] >> c) & 1:
                    reached[r, c] = True
                    lab[r, c] = lv[(x >> (8 * i)) & 0xFF]
    return True, lab, reached, k


def visit_bfs(win, arcs):
    """Returns (labels, nbm, took_fallback)."""
    win64 = np.asarray(win).astype(np.int64)
    start = win64[1:33, 1:33]
    ok, lab, reached, _ = bfs_levels(win, arcs)
    if ok:
        viol = np.where(reached, start < lab, start != DINF)
        ok = not viol.any()
    if not ok:
        labels, nbm, _ = visit_sweeps(win, arcs)
        return labels, nbm, True
    new = np.minimum(start, lab)
    return new.astype(np.int32), _nbm(start, new, True), False
