"""Pins, without any device code, which path of ggc_slic_enforce_connectivity each case of tests/connectivity_cases.py must
take: the components of every raw label are counted with scipy.ndimage.label and set against min_size, max_size and the
capacity of the on-chip queue.  tests/test_connectivity_tiles_gpu.py asserts these paths on the device."""
import collections

import numpy as np

import connectivity_cases as cc


def test_fuzz_paths_are_the_pinned_ones_and_cover_both_paths():
    paths = [cc.expected_path(*cc.fuzz_case(k)) for k in range(40)]
    assert tuple(paths) == cc.FUZZ_PATHS
    n = collections.Counter(paths)
    assert n["tiles"] >= 25 and n["rounds"] >= 5, n


def test_fuzz_cases_have_the_shapes_and_kinds_asked_for():
    for k in range(40):
        raw, mn, mx = cc.fuzz_case(k)
        b, h, w = raw.shape
        assert 2 <= b <= 4 and 1 <= h <= 80 and 1 <= w <= 150
        assert mn in (4, 20, 100, 300) and mx in (3 * mn, cc.BIG)


def test_hand_cases_take_the_paths_they_are_built_for():
    for name, (raw, mn, mx, path) in cc.hand_cases().items():
        assert cc.expected_path(raw, mn, mx) == path, name


def test_hand_shapes_are_what_their_names_say():
    from scipy import ndimage
    sp = cc.spiral(3 * cc.TH + 3, 3 * cc.TW + 5)
    ys, xs = np.nonzero(sp == 1)
    assert ndimage.label(sp == 1)[1] == 1 and len(set(zip(ys // cc.TH, xs // cc.TW))) >= 6
    u = cc.u_shape()
    assert ndimage.label(u == 1)[1] == 1 and ndimage.label(u[:cc.TH] == 1)[1] == 2       # two arms in the first tile row
    lc = cc.last_column_root()
    assert ndimage.label(lc == 1)[1] == 1 and np.flatnonzero(lc.ravel() == 1)[0] % lc.shape[1] >= 2 * cc.TW
    st = cc.blobs_on_stripes(True)
    assert int((st == 10).sum()) == 40 and int((st == 11).sum()) == 39
    assert set(np.unique(st[cc.TH - 1:cc.TH + 1, cc.TW - 1:cc.TW + 1])) == {9}           # the blob on the tile corner
    for n in (cc.QCAP - 1, cc.QCAP, cc.QCAP + 1):
        s = cc.serpentine(48, 40, n)
        assert int((s == 1).sum()) == n
        assert cc.expected_path(s[None], cc.QCAP + 50, cc.BIG) == ("spill" if n > cc.QCAP else "tiles")
