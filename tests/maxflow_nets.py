"""Grid networks built to break the device max-flow, and a max-flow/min-cut certificate of its final state.

A network is one image: tw (n_steps, H, W) int32 t-link differences (source minus sink; later steps only change tw) and
nw (4, H, W) int32 undirected n-links towards left, up-left, up, up-right: the CPU oracle's plane convention
(oracle.grid_maxflow).  to_device() stacks a batch into ggc_grid_maxflow's layout, solve() runs it on the device.

Each family aims at one mechanism of the solver (32x32 relabel tiles, 32x8 dense push tiles, 32x16 / 32x32 asynchronous
push tiles):
  random              the oracle test's distribution: the baseline
  serpentine          a 1-pixel corridor zig-zagging between zero-capacity walls, source at one end, sink at the other and
                      one bottleneck in between: relabel fronts across hundreds of tiles, visits that stop short of their
                      fixpoint, long push chains, excess trapped behind the saturated bottleneck
  corner_gates        walls on every tile border, crossable only by the diagonal links at tile corners: halo corners
  border_bottlenecks  source and sink tiles whose min cut is exactly the links on tile borders: stale arc masks there
  extremes            |tw| = 2^27, nw = 2^24 (ggc_grid_maxflow's bounds): int32 excess at its largest
  degenerate          no links, no t-links, one sign only, garbage in the planes that point outside the image
  warm                4 steps on one nw, each resampling about 20 % of tw (signs flip), a definite subset fixed
"""
import numpy as np

PLANE_OFF = [(0, -1), (-1, -1), (-1, 0), (-1, 1)]   # (dy, dx) of planes left, up-left, up, up-right
# arcs of the device state, direction order of csrc/ggc_gc.h: (dy, dx, plane, the plane's owner is the arc's head)
DIRS = [(0, -1, 0, False), (0, 1, 0, True), (-1, 0, 2, False), (1, 0, 2, True),
        (-1, -1, 1, False), (1, 1, 1, True), (-1, 1, 3, False), (1, -1, 3, True)]
TW_MAX, NW_MAX = 1 << 27, 1 << 24

VARIANTS = {
    "random": ["dense", "sparse_tw"],
    "serpentine": ["mid_bottleneck"],
    "corner_gates": ["gates"],
    "border_bottlenecks": ["tiles_32x8", "tiles_32x32"],
    "extremes": ["checker", "stripes", "one_sink", "one_source"],
    "degenerate": ["no_links", "no_tlinks", "all_source", "all_sink", "outside_garbage"],
    "warm": ["resample"],
}


def in_image(h, w):
    """(4, H, W) bool: the plane's link points to a pixel of the image."""
    m = np.zeros((4, h, w), bool)
    for k, (dy, dx) in enumerate(PLANE_OFF):
        m[k, max(0, -dy):h - max(0, dy), max(0, -dx):w - max(0, dx)] = True
    return m


def _zero_outside(nw):
    return np.where(in_image(*nw.shape[1:]), nw, 0).astype(np.int32)


def _random(h, w, rng, variant):
    tw = rng.integers(-60, 61, size=(h, w))
    tw[rng.random((h, w)) < (0.3 if variant == "dense" else 0.9)] = 0
    nw = rng.integers(0, 25, size=(4, h, w))
    return tw[None], nw


def _serpentine(h, w, rng, variant):
    """Corridor rows 0, 2, 4, ... joined at alternating ends through the odd rows; every other link is zero."""
    nw = np.zeros((4, h, w), np.int64)
    tw = np.zeros((h, w), np.int64)
    cap = 1000
    path = []
    rows = list(range(0, h, 2))
    for j, y in enumerate(rows):
        xs = range(w) if j % 2 == 0 else range(w - 1, -1, -1)
        if j > 0:                                          # the connector pixel below the end of the previous row
            xc = w - 1 if j % 2 == 1 else 0
            path.append((y - 1, xc))
        path.extend((y, x) for x in xs)
    for (y0, x0), (y1, x1) in zip(path, path[1:]):
        c = cap + int(rng.integers(0, 50))
        if y0 == y1:
            nw[0, y0, max(x0, x1)] = c                     # left link of the right pixel
        else:
            nw[2, max(y0, y1), x0] = c                     # up link of the lower pixel
    if len(path) >= 2:
        # the bottleneck: the link into the middle pixel of the corridor
        (y0, x0), (y1, x1) = path[len(path) // 2 - 1], path[len(path) // 2]
        if y0 == y1:
            nw[0, y0, max(x0, x1)] = 7
        else:
            nw[2, max(y0, y1), x0] = 7
    tw[path[0]] = 50 * cap
    tw[path[-1]] = -50 * cap
    return tw[None], nw


def _corner_gates(h, w, rng, variant):
    """32x8 cells (which tile the 32x32, 32x16 and 32x8 tiles too); a link may cross a cell border only diagonally at a
    corner.  Sources in the top-left cells, sinks in the bottom-right ones, a little noise everywhere."""
    ys, xs = np.mgrid[0:h, 0:w]
    cy, cx = ys // 8, xs // 32
    nw = np.zeros((4, h, w), np.int64)
    for k, (dy, dx) in enumerate(PLANE_OFF):
        qcy, qcx = (ys + dy) // 8, (xs + dx) // 32
        same = (qcy == cy) & (qcx == cx)
        corner = (qcy != cy) & (qcx != cx)                 # only a diagonal link can change both
        c = np.where(same, rng.integers(200, 400, size=(h, w)), 0)
        c = np.where(corner, rng.integers(1, 40, size=(h, w)), c)
        nw[k] = c
    tw = rng.integers(-3, 4, size=(h, w))
    far = (cy + cx)
    tw[far == 0] += 500
    tw[far == far.max()] -= 500
    if far.max() >= 2:
        tw[far == far.max() - 1] -= 300                    # (the other parity of cells, reached through other corners)
        tw[far == 1] += 300
    return tw[None], nw


def _border_bottlenecks(h, w, rng, variant):
    """Tiles labelled source or sink at random; strong links inside a tile, weak ones across its border: the min cut is
    made of border links, which saturate."""
    th = 8 if variant == "tiles_32x8" else 32
    ys, xs = np.mgrid[0:h, 0:w]
    cy, cx = ys // th, xs // 32
    lab = rng.integers(0, 2, size=(cy.max() + 1, cx.max() + 1))
    lab[0, 0], lab[-1, -1] = 1, 0
    sign = np.where(lab[cy, cx] == 1, 1, -1)
    tw = sign * rng.integers(50, 200, size=(h, w))
    tw[rng.random((h, w)) < 0.5] = 0
    nw = np.zeros((4, h, w), np.int64)
    for k, (dy, dx) in enumerate(PLANE_OFF):
        same = ((ys + dy) // th == cy) & ((xs + dx) // 32 == cx)
        nw[k] = np.where(same, rng.integers(5000, 9000, size=(h, w)), rng.integers(1, 6, size=(h, w)))
    return tw[None], nw


def _extremes(h, w, rng, variant):
    ys, xs = np.mgrid[0:h, 0:w]
    if variant == "checker":
        tw = np.where((ys + xs) % 2 == 0, TW_MAX, -TW_MAX)
    elif variant == "stripes":
        tw = np.where(xs % 3 == 0, -TW_MAX, TW_MAX)
    elif variant == "one_sink":                            # everything drains into one pixel
        tw = np.full((h, w), TW_MAX); tw[h // 2, w // 2] = -TW_MAX
    else:                                                  # one source feeds everything
        tw = np.full((h, w), -TW_MAX); tw[h // 2, w // 2] = TW_MAX
    nw = np.full((4, h, w), NW_MAX)
    return tw[None], nw


def _degenerate(h, w, rng, variant):
    tw, nw = _random(h, w, rng, "dense")
    tw = tw[0]
    if variant == "no_links":
        nw = np.zeros_like(nw)
    elif variant == "no_tlinks":
        tw = np.zeros_like(tw)
    elif variant == "all_source":
        tw = np.abs(tw) + 1
    elif variant == "all_sink":
        tw = -np.abs(tw) - 1
    else:                                                  # planes that point outside: never read
        junk = rng.choice(np.array([-(1 << 31), -1, 1 << 30, (1 << 31) - 1, NW_MAX + 1]), size=nw.shape)
        nw = np.where(in_image(h, w), nw, junk)
        return tw[None], nw                                # (kept: the junk is the point)
    return tw[None], nw


def _warm(h, w, rng, variant, n_steps=4):
    """One nw, GrabCut-like t-links: a definite subset pinned at +-lambda, the rest resampled ~20 % per step."""
    lam = 30000
    nw = rng.integers(0, 4000, size=(4, h, w))
    tw = rng.integers(-8000, 8001, size=(h, w))
    definite = rng.random((h, w)) < 0.3
    tw[definite] = np.where(rng.random(int(definite.sum())) < 0.5, lam, -lam)
    steps = [tw.copy()]
    for _ in range(n_steps - 1):
        resample = (rng.random((h, w)) < 0.2) & ~definite
        tw = tw.copy()
        tw[resample] = -tw[resample] + rng.integers(-500, 501, size=int(resample.sum()))   # mostly a sign flip
        steps.append(tw)
    return np.stack(steps), nw


_GEN = {"random": _random, "serpentine": _serpentine, "corner_gates": _corner_gates,
        "border_bottlenecks": _border_bottlenecks, "extremes": _extremes, "degenerate": _degenerate, "warm": _warm}


def make(family, variant, h, w, seed=0):
    """-> tw (n_steps, H, W) int32, nw (4, H, W) int32.  Out-of-image links are zero except in degenerate/outside_garbage."""
    rng = np.random.default_rng([seed, h, w, list(_GEN).index(family), VARIANTS[family].index(variant)])
    tw, nw = _GEN[family](h, w, rng, variant)
    if not (family == "degenerate" and variant == "outside_garbage"):
        nw = _zero_outside(nw)
    return np.ascontiguousarray(tw, np.int32), np.ascontiguousarray(nw, np.int32)


# ------------------------------------------------------------------------------------------------ device
def to_device(nets):
    """[(tw (S,H,W), nw (4,H,W))] of one shape and step count -> tw (S,B,H,W), nw (4,B,H,W) as in ggc_grid_maxflow."""
    tw = np.ascontiguousarray(np.stack([t for t, _ in nets], axis=1), np.int32)
    nw = np.ascontiguousarray(np.stack([n for _, n in nets], axis=1), np.int32)
    return tw, nw


def solve(ctx, nets, residual=True):
    """Runs ggc_grid_maxflow on a batch of networks -> source_side (S,B,H,W) u8, residual (B,H,W,10) i32 or None."""
    import torch
    from gcn_grabcut import _native
    tw, nw = to_device(nets)
    s, b, h, w = tw.shape
    dtw, dnw = torch.as_tensor(tw).cuda(), torch.as_tensor(nw).cuda()
    side = torch.full((s, b, h, w), 255, dtype=torch.uint8, device="cuda")
    res = torch.full((b, h, w, 10), -(1 << 31), dtype=torch.int32, device="cuda") if residual else None
    ctx.call("ggc_grid_maxflow", _native.current_stream(0), b, h, w, s, dtw.data_ptr(), dnw.data_ptr(), side.data_ptr(),
             res.data_ptr() if residual else None)
    return side.cpu().numpy(), (res.cpu().numpy() if residual else None)


# ------------------------------------------------------------------------------------------------ certificate
def _arc_caps(nw):
    """(H, W, 8) int64 capacity of every arc of the device state (0 for arcs that leave the image)."""
    h, w = nw.shape[1:]
    nw = np.where(in_image(h, w), nw.astype(np.int64), 0)
    c = np.zeros((h, w, 8), np.int64)
    for d, (dy, dx, k, head_owns) in enumerate(DIRS):
        if not head_owns:
            c[:, :, d] = nw[k]
        else:                                              # the link lives in the plane of the head q = p + (dy, dx)
            c[max(0, -dy):h - max(0, dy), max(0, -dx):w - max(0, dx), d] = \
                nw[k, max(0, dy):h - max(0, -dy), max(0, dx):w - max(0, -dx)]
    return c


def _shift(a, dy, dx):
    """b[y, x] = a[y + dy, x + dx], zero outside."""
    h, w = a.shape[:2]
    b = np.zeros_like(a)
    b[max(0, -dy):h - max(0, dy), max(0, -dx):w - max(0, dx)] = a[max(0, dy):h - max(0, -dy), max(0, dx):w - max(0, -dx)]
    return b


def reaches_sink(rc, snk):
    """(H, W) bool: the pixel reaches a pixel with residual sink capacity through arcs with rc > 0."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import breadth_first_order
    h, w = snk.shape
    n = h * w
    idx = np.arange(n).reshape(h, w)
    rows, cols = [], []                                    # reversed arcs q -> p for every residual arc p -> q
    for d, (dy, dx, _, _) in enumerate(DIRS):
        ok = (rc[:, :, d] > 0) & (_shift(np.ones((h, w), bool), dy, dx))
        p = idx[ok]
        q = p + dy * w + dx
        rows.append(q); cols.append(p)
    t = n
    sinks = idx[snk > 0]
    rows.append(np.full(sinks.size, t)); cols.append(sinks)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    g = sp.csr_matrix((np.ones(rows.size, np.int8), (rows, cols)), shape=(n + 1, n + 1))
    order = breadth_first_order(g, t, directed=True, return_predecessors=False)
    r = np.zeros(n + 1, bool)
    r[order] = True
    return r[:n].reshape(h, w)


def cut_capacity(tw, nw, source_side):
    """Capacity of the s-t cut (source_side, rest) of the network (tw, nw), in int64."""
    tw = tw.astype(np.int64)
    s = source_side.astype(bool)
    c = _arc_caps(nw)
    cap = int(np.maximum(-tw, 0)[s].sum()) + int(np.maximum(tw, 0)[~s].sum())
    for d, (dy, dx, _, _) in enumerate(DIRS):
        head_sink = ~_shift(s, dy, dx) & _shift(np.ones_like(s), dy, dx)
        cap += int(c[:, :, d][s & head_sink].sum())
    return cap


def certify(tw, nw, source_side, residual, flow, cold=False):
    """Asserts that residual (H, W, 10) is a maximum preflow of (tw, nw), that source_side is its canonical cut (the pixels
    that cannot reach the sink) and that the cut's capacity is `flow`, the oracle's max-flow value.  int64 throughout."""
    tw = np.asarray(tw, np.int64)
    res = np.asarray(residual, np.int64)
    rc, ex, snk = res[:, :, :8], res[:, :, 8], res[:, :, 9]
    h, w = tw.shape
    c = _arc_caps(nw)
    inside = np.stack([_shift(np.ones((h, w), bool), dy, dx) for dy, dx, _, _ in DIRS], axis=2)
    # 1. residual arcs are non-negative; an arc that leaves the image has none
    assert (rc >= 0).all(), f"negative residual arc at {np.argwhere(rc < 0)[:4].tolist()}"
    assert (rc[~inside] == 0).all(), "residual capacity on an arc that leaves the image"
    # 2. both arcs of a link hold its capacity twice
    for d, (dy, dx, _, _) in enumerate(DIRS):
        back = _shift(rc[:, :, d ^ 1], dy, dx)
        bad = inside[:, :, d] & (rc[:, :, d] + back != 2 * c[:, :, d])
        assert not bad.any(), f"pair sum of direction {d} broken at {np.argwhere(bad)[:4].tolist()}"
    # 3. flow conservation with the terminal balance
    inflow = (rc - c).sum(axis=2)
    bad = ex - snk != tw + inflow
    assert not bad.any(), f"balance ex - snk != tw + inflow at {np.argwhere(bad)[:4].tolist()}"
    assert (ex >= 0).all() and (snk >= 0).all(), "negative excess or sink capacity"
    assert (np.minimum(ex, snk) == 0).all(), "a pixel keeps both excess and sink capacity"
    # 4. a maximum preflow: no excess can still reach the sink
    reach = reaches_sink(rc, snk)
    bad = (ex > 0) & reach
    assert not bad.any(), f"preflow not maximal: excess reaches the sink from {np.argwhere(bad)[:4].tolist()}"
    # 5. the canonical cut
    bad = source_side.astype(bool) != ~reach
    assert not bad.any(), f"source_side differs from the residual reachability at {np.argwhere(bad)[:4].tolist()}"
    # 6. min cut == max flow
    cap = cut_capacity(tw, nw, source_side)
    assert cap == flow, f"cut capacity {cap} != flow value {flow}"
    if cold:
        drained = int(np.maximum(-tw, 0).sum() - snk.sum())
        assert drained == flow, f"flow into the sink {drained} != flow value {flow}"


def state_from_scipy(tw, nw):
    """A maximum preflow in the device's state layout, from scipy's maximum_flow -> (residual (H,W,10) int64, flow)."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import maximum_flow
    tw = np.asarray(tw, np.int64)
    h, w = tw.shape
    n = h * w
    s, t = n, n + 1
    idx = np.arange(n).reshape(h, w)
    c = _arc_caps(nw)
    rows, cols, caps = [], [], []
    for d, (dy, dx, _, _) in enumerate(DIRS):
        ok = c[:, :, d] > 0
        rows.append(idx[ok]); cols.append(idx[ok] + dy * w + dx); caps.append(c[:, :, d][ok])
    pos, neg = tw > 0, tw < 0
    rows += [np.full(int(pos.sum()), s), idx[neg]]
    cols += [idx[pos], np.full(int(neg.sum()), t)]
    caps += [tw[pos], -tw[neg]]
    g = sp.csr_matrix((np.concatenate(caps).astype(np.int32), (np.concatenate(rows), np.concatenate(cols))), shape=(n + 2, n + 2))
    r = maximum_flow(g, s, t)
    f = r.flow.tocsr()                                     # antisymmetric net flow
    res = np.zeros((h, w, 10), np.int64)
    for d, (dy, dx, _, _) in enumerate(DIRS):
        ok = _shift(np.ones((h, w), bool), dy, dx)
        p = idx[ok]
        fpq = np.asarray(f[p, p + dy * w + dx]).ravel()
        res[:, :, d][ok] = c[:, :, d][ok] - fpq
    f_sp = np.asarray(f[s, np.arange(n)].todense()).ravel().reshape(h, w)
    f_pt = np.asarray(f[np.arange(n), t].todense()).ravel().reshape(h, w)
    res[:, :, 8] = np.where(pos, tw - f_sp, 0)             # source flow that never left: trapped excess
    res[:, :, 9] = np.where(neg, -tw - f_pt, 0)
    return res, int(r.flow_value)
