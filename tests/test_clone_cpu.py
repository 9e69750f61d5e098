"""The cloning rule of include/ggc.h O5 / O6 without a GPU: the restatement (tests/clone_ref.py) against the exact sparse
solve, the exact zero of an identity clone, the mixed rule's tie, the images that are not solved, the rounding rule's
margin, the host argument checks, the header and composite.py's argument parsing.  The cases defined here are the ones
test_clone_gpu.py runs on the device."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import clone_ref as ref

ROOT = Path(__file__).resolve().parent.parent
TOL = 1e-9                                        # the tolerance of the agreement tests
AGREE_LEVELS = 1e-3                               # |PCG - exact| on Omega, in levels: a condition, not a measurement
HALF_MARGIN = 1e-3                                # a pixel this close to a half-integer may round either way
MAX_ITER = 5000


def _noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def _disk(h, w, cy, cx, r):
    y, x = np.mgrid[:h, :w]
    return ((y - cy) ** 2 + (x - cx) ** 2 <= r * r).astype(np.uint8)


def case(name):
    """-> (source (Hs,Ws,3), mask (Hs,Ws), target (H,W,3), offset (row, col)); random-noise colours, the worst case for
    the solution's range."""
    if name == "overhang":                        # 1: the source overhangs the target on every side; Omega the whole target
        return _noise((9, 9, 3), 1), np.ones((9, 9), np.uint8), _noise((5, 7, 3), 2), (-2, -1)
    if name == "disk":                            # 2: 2 x 3 tiles, partial; Omega cut by the top and right border
        return _noise((31, 31, 3), 3), _disk(31, 31, 15, 15, 14), _noise((33, 47, 3), 4), (-7, 20)
    if name == "all_tiles":                       # 3: 81 tiles listed: the second stride of the per-image sum
        return _noise((128, 128, 3), 5), np.ones((128, 128), np.uint8), _noise((130, 130, 3), 6), (1, 1)
    if name == "ring":                            # 4: a hole
        m = _disk(64, 64, 32, 32, 25) - _disk(64, 64, 32, 32, 10)
        return _noise((64, 64, 3), 7), m, _noise((64, 64, 3), 8), (0, 0)
    if name == "lines":                           # 5: one pixel wide, along and across tile edges, crossing at a corner
        m = np.zeros((40, 40), np.uint8)
        m[16, 3:37] = 1                           # the first row of the second tile row
        m[2:38, 15] = 1                           # the last column of the first tile column
        m[31, 10:34] = 1                          # the last row of the second tile row
        m[5:30, 32] = 1                           # the first column of the third tile column
        return _noise((40, 40, 3), 9), m, _noise((40, 40, 3), 10), (0, 0)
    if name == "pixel":                           # 6: the smallest solvable region
        m = np.zeros((20, 20), np.uint8)
        m[16, 16] = 1
        return _noise((20, 20, 3), 11), m, _noise((20, 20, 3), 12), (0, 0)
    if name == "empty":                           # 7
        return _noise((20, 20, 3), 13), np.zeros((20, 20), np.uint8), _noise((20, 24, 3), 14), (0, 3)
    if name == "whole":                           # 8
        return _noise((20, 24, 3), 15), np.ones((20, 24), np.uint8), _noise((20, 24, 3), 16), (0, 0)
    if name == "identity":                        # 9: cloned onto itself
        t = _noise((40, 40, 3), 17)
        return t.copy(), _disk(40, 40, 20, 18, 13), t, (0, 0)
    if name == "disk48x64":
        return _noise((48, 64, 3), 18), _disk(48, 64, 24, 30, 20), _noise((48, 64, 3), 19), (0, 0)
    raise KeyError(name)


SOLVED = ("disk", "all_tiles", "ring", "lines", "pixel", "disk48x64")
ALL = ("overhang",) + SOLVED[:5] + ("empty", "whole", "identity")


def batch_members():
    """Eight images of one shape (source 40 x 50, target 33 x 47) with their own offsets: the kinds of cases 2, 4, 6, 7,
    8 and 9, and two noise masks.  -> (sources, masks, targets, offsets)."""
    hs, ws, h, w = 40, 50, 33, 47
    src = [_noise((hs, ws, 3), 30 + k) for k in range(8)]
    tgt = [_noise((h, w, 3), 40 + k) for k in range(8)]
    rng = np.random.default_rng(50)
    ring = _disk(hs, ws, 18, 22, 15) - _disk(hs, ws, 18, 22, 6)
    one = np.zeros((hs, ws), np.uint8)
    one[20, 21] = 1
    masks = [_disk(hs, ws, 20, 25, 14), ring, one, np.zeros((hs, ws), np.uint8), np.ones((hs, ws), np.uint8),
             _disk(hs, ws, 19, 24, 12), (rng.random((hs, ws)) < 0.5).astype(np.uint8),
             (rng.random((hs, ws)) < 0.9).astype(np.uint8)]
    offsets = [(-7, 20), (-2, -1), (-4, -5), (3, 3), (-3, -2), (-3, -2), (0, 0), (-9, 4)]
    src[5][3:3 + h, 2:2 + w] = tgt[5]             # the identity clone: the source holds the target at its offset
    return np.stack(src), np.stack(masks), np.stack(tgt), np.array(offsets, np.int32)


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("name", SOLVED)
def test_restatement_pcg_agrees_with_the_exact_solve_and_the_rounding_margin_is_small(name, mixed):
    s, m, t, off = case(name)
    sys_ = ref.assemble(s, m, t, off, mixed)
    n = len(sys_["g"])
    assert 0 < n < t.shape[0] * t.shape[1]
    assert np.abs(sys_["A"] - sys_["A"].T).max() == 0
    want = ref.exact(sys_)
    f, it, rel = ref.pcg(sys_, MAX_ITER, TOL)
    err = np.abs(f - want).max()
    near_half = np.abs(np.clip(want, 0, 255) % 1.0 - 0.5) <= HALF_MARGIN
    print(f"{name} mixed={mixed}: |Omega| {n}, iterations {it}, rel {rel:.2e}, |pcg - exact| {err:.2e} levels, range "
          f"{want.min():.0f}..{want.max():.0f}, values within {HALF_MARGIN} of a half {near_half.sum()} of {3 * n}")
    assert 1 <= it < MAX_ITER and rel <= TOL
    assert err <= AGREE_LEVELS
    assert near_half.any(axis=1).sum() < 0.01 * n                 # the pixels the rounding test of the GPU excludes
    res, res0 = ref.residual_norms(sys_, _raw(t, sys_, f))
    assert res <= 2.0 * TOL * res0


def _raw(t, sys_, f):
    raw = t.astype(np.float64)
    raw[sys_["omega"]] = f
    return raw


def test_degrees_are_2_and_3_where_omega_meets_the_targets_border():
    s, m, t, off = case("disk")
    sys_ = ref.assemble(s, m, t, off, False)
    assert set(np.unique(sys_["deg"])) == {2, 3, 4}
    assert sys_["omega"][0].any() and sys_["omega"][:, -1].any()


def test_identity_clone_has_an_exactly_zero_first_residual():
    s, m, t, off = case("identity")
    for mixed in (False, True):
        sys_ = ref.assemble(s, m, t, off, mixed)
        assert not ref.first_residual(sys_).any()
        out = ref.clone(s, m, t, off, mixed, MAX_ITER, TOL)
        assert out["iters"] == 0 and out["rel"] == 0.0 and np.array_equal(out["composite"], t)
    srcs, masks, tgts, offs = batch_members()
    assert not ref.first_residual(ref.assemble(srcs[5], masks[5], tgts[5], offs[5], True)).any()


def test_mixed_rule_takes_the_larger_gradient_and_a_tie_goes_to_the_source():
    # one unknown pixel with four known neighbours: b = sum t_q + sum v_pq, f = b / 4
    t = np.full((3, 3, 3), 100, np.uint8)
    t[1, 1] = 100
    t[0, 1] = 90                                   # d_t towards the top neighbour: +10
    s = np.full((3, 3, 3), 50, np.uint8)
    s[0, 1] = 60                                   # d_s towards the top neighbour: -10, a tie in magnitude
    s[1, 0] = 30                                   # d_s towards the left neighbour: +20 against d_t = 0
    t[1, 2] = 70                                   # d_t towards the right neighbour: +30 against d_s = 0
    m = np.zeros((3, 3), np.uint8)
    m[1, 1] = 1
    plain = ref.assemble(s, m, t, (0, 0), False)
    mixed = ref.assemble(s, m, t, (0, 0), True)
    known = 90 + 100 + 70 + 100
    assert plain["b"].tolist() == [[known + (-10 + 20 + 0 + 0)] * 3]
    assert mixed["b"].tolist() == [[known + (-10 + 20 + 30 + 0)] * 3]           # the tie kept d_s = -10, not d_t = +10
    assert np.allclose(ref.exact(mixed), (known + 40) / 4.0)


def test_a_neighbour_without_a_source_pixel_has_no_source_gradient():
    t = _noise((4, 4, 3), 60)
    s = _noise((2, 2, 3), 61)
    m = np.ones((2, 2), np.uint8)
    sys_ = ref.assemble(s, m, t, (1, 1), False)
    g = s.astype(np.int64)
    tt = t.astype(np.int64)
    # Omega's first pixel (1, 1): up and left lie outside the source, right and down inside it and in Omega
    want = tt[0, 1] + tt[1, 0] + (g[0, 0] - g[0, 1]) + (g[0, 0] - g[1, 0])
    assert np.array_equal(sys_["b"][0], want)


def test_empty_and_whole_target_omegas_are_not_solved():
    s, m, t, off = case("empty")
    out = ref.clone(s, m, t, off, False, MAX_ITER, TOL)
    assert out["n_omega"] == 0 and out["iters"] == 0 and out["rel"] == 0.0 and np.array_equal(out["composite"], t)
    for name in ("whole", "overhang"):
        s, m, t, off = case(name)
        out = ref.clone(s, m, t, off, True, MAX_ITER, TOL)
        h, w = t.shape[:2]
        assert out["n_omega"] == h * w and out["iters"] == 0 and out["rel"] == 0.0
        assert np.array_equal(out["composite"], s[-off[0]:h - off[0], -off[1]:w - off[1]])


def test_alpha_over_restatement():
    bg = _noise((5, 7, 3), 70)
    rgba = _noise((9, 9, 4), 71)
    rgba[0:3, :, 3] = 0
    rgba[3:6, :, 3] = 255
    out = ref.over(rgba, bg, (-2, -1))
    assert np.array_equal(out[0], bg[0]) and np.array_equal(out[1:4], rgba[3:6, 1:8, :3])
    a, c, b = int(rgba[6, 3, 3]), rgba[6, 3, :3].astype(int), bg[4, 2].astype(int)     # out[y, x] takes rgba[y + 2, x + 1]
    assert np.array_equal(out[4, 2], (a * c + (255 - a) * b + 127) // 255)
    assert np.array_equal(ref.over(rgba, bg, (5, 0)), bg) and np.array_equal(ref.over(rgba, bg, (0, -9)), bg)


# ---------------------------------------------------------------- the host
BAD_CLONE = [dict(max_iter=0), dict(max_iter=100001), dict(max_iter=2.5), dict(tol=0.0), dict(tol=1.0),
             dict(tol=float("nan")), dict(mixed=2), dict(offset=(1.5, 0)), dict(offset=(0, 40000)), dict(offset=(1, 2, 3))]


@pytest.fixture()
def no_native(monkeypatch):
    """Any native call after this is an error: the checks under test come first."""
    from gcn_grabcut import _engine

    def boom(*a, **k):
        raise AssertionError("the engine was reached before the arguments were checked")
    monkeypatch.setattr(_engine, "get_engine", boom)


@pytest.mark.parametrize("kw", BAD_CLONE)
def test_seamless_clone_refuses_bad_arguments_before_any_native_call(no_native, kw):
    from gcn_grabcut import seamless_clone
    s, m, t, _ = case("pixel")
    with pytest.raises(ValueError):
        seamless_clone(s, m, t, **kw)


def test_public_entries_refuse_bad_shapes_and_dtypes_before_any_native_call(no_native):
    from gcn_grabcut import Clone, composite_over, composite_over_batch, seamless_clone, seamless_clone_batch
    s, m, t, _ = case("pixel")
    with pytest.raises(ValueError):
        seamless_clone(s, m[:, :5], t)
    with pytest.raises(ValueError):
        seamless_clone(s.astype(np.float32), m, t)
    with pytest.raises(ValueError):
        seamless_clone(s, m.astype(np.float32), t)
    with pytest.raises(ValueError):
        seamless_clone(s, m, t[..., :2])
    with pytest.raises(ValueError):
        seamless_clone_batch(s[None], m[None], np.stack([t, t]))
    with pytest.raises(ValueError):
        seamless_clone_batch(s[None], m[None], t[None], clone="mixed")
    rgba = np.zeros((4, 4, 4), np.uint8)
    with pytest.raises(ValueError):
        composite_over(rgba[..., :3], t)
    with pytest.raises(ValueError):
        composite_over(rgba.astype(np.int32), t)
    with pytest.raises(ValueError):
        composite_over(rgba, t, offset=(0, -32769))
    with pytest.raises(ValueError):
        composite_over_batch(np.stack([rgba, rgba]), t[None])
    with pytest.raises(ValueError):
        Clone(max_iter=0)
    with pytest.raises(ValueError):
        Clone(mixed=1)
    c = Clone()
    assert c.args() == (False, 10000, 1e-7)
    with pytest.raises(Exception):
        c.tol = 1e-3                               # frozen


def test_composite_onto_refuses_a_bad_method_before_any_native_call(no_native):
    from gcn_grabcut import SegmentationResult
    z = np.zeros((4, 4), np.uint8)
    r = SegmentationResult(image=np.zeros((4, 4, 3), np.uint8), binary_mask=z, trimap=z, segments=z,
                           overlay=np.zeros((4, 4, 3), np.uint8), rgba=np.zeros((4, 4, 4), np.uint8))
    with pytest.raises(ValueError, match="method"):
        r.composite_onto(np.zeros((6, 6, 3), np.uint8), method="poisson")
    with pytest.raises(ValueError, match="full"):
        r.composite_onto(np.zeros((6, 6, 3), np.uint8), full=True)


def test_header_declares_both_entries():
    header = (ROOT / "include" / "ggc.h").read_text()
    assert int(re.search(r"#define GGC_VERSION (\d+)", header).group(1)) >= 411
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint ggc_composite_over\s*\(", body) and re.search(r"\bint ggc_poisson_clone\s*\(", body)
    from gcn_grabcut import _native
    assert len(_native.SIGNATURES["ggc_composite_over"]) == 11 and len(_native.SIGNATURES["ggc_poisson_clone"]) == 19


def _composite_module():
    sys.path.insert(0, str(ROOT))
    import composite
    return composite


def test_composite_py_argument_parsing():
    comp = _composite_module()
    parser = comp.build_parser()
    a = parser.parse_args(["--cutout", "x_cutout.png", "--background", "b.jpg", "--at=-3,12", "--save", "out.png"])   # a negative row needs the = form
    comp.check_args(parser, a)
    assert a.method == "over" and a.at == (-3, 12) and a.save == "out.png"
    a = parser.parse_args(["--image", "x.jpg", "--mask", "x_mask.png", "--background", "b.jpg", "--method", "mixed"])
    comp.check_args(parser, a)
    assert a.method == "mixed" and a.at == (0, 0)
    a = parser.parse_args(["--image", "x.jpg", "--mask", "x_mask.png", "--background", "b.jpg"])
    comp.check_args(parser, a)
    assert a.method == "seamless"
    for bad in (["--cutout", "c.png", "--background", "b.jpg", "--method", "seamless"],
                ["--image", "x.jpg", "--background", "b.jpg"],
                ["--image", "x.jpg", "--mask", "m.png", "--background", "b.jpg", "--method", "over"],
                ["--cutout", "c.png", "--mask", "m.png", "--background", "b.jpg"],
                ["--cutout", "c.png", "--background", "b.jpg", "--at", "1;2"],
                ["--cutout", "c.png", "--background", "b.jpg", "--at", "1,40000"],
                ["--cutout", "c.png"]):
        with pytest.raises(SystemExit):
            comp.check_args(parser, parser.parse_args(bad))
