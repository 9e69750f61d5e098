"""The Python layer of the distance transform and the mask modifiers: radius conversions and refusals, all of which happen
before any device call, the header's section and the command lines' new options.  No device is needed."""
import dataclasses
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
M = np.zeros((4, 5), np.uint8)
MAX2 = 2 * 16384 ** 2


def test_radius_is_floor_of_its_square_and_radius2_is_exact():
    from gcn_grabcut import ModifyMask
    assert ModifyMask("grow", 3).args() == (0, 9, 0, False)
    assert ModifyMask("shrink", 1.5, border_background=True).args() == (1, 2, 0, True)          # floor(2.25): the 8-neighbourhood
    assert ModifyMask("open", radius2=2).args() == (3, 2, 0, False)
    assert ModifyMask("close", 0).args() == (4, 0, 0, False)
    assert ModifyMask("border", 2).args() == (2, 4, 4, False)                                   # outer None: outer = inner
    assert ModifyMask("border", 2, 3.2).args() == (2, 4, 10, False)
    assert ModifyMask("trimap", 0, 3).args() == (5, 0, 9, False)
    assert ModifyMask("trimap", radius2=(5, 0)).args() == (5, 5, 0, False)
    assert ModifyMask("trimap", radius2=7).args() == (5, 7, 7, False)
    assert ModifyMask("GROW", np.int64(4)).args() == (0, 16, 0, False) and ModifyMask(1, np.float32(2.0)).args()[1] == 4
    assert ModifyMask("grow", radius2=MAX2).args()[1] == MAX2 and ModifyMask("grow", 16384).args()[1] == 16384 ** 2
    with pytest.raises(dataclasses.FrozenInstanceError):
        ModifyMask("grow", 1).radius = 2


@pytest.mark.parametrize("bad", [dict(radius=-1), dict(radius=-0.5), dict(radius=float("nan")), dict(radius=float("inf")),
                                 dict(radius=1e200), dict(radius=23171), dict(radius2=MAX2 + 1), dict(radius2=-1),
                                 dict(radius2=2.0), dict(radius2=True), dict(radius=1, radius2=1), dict(), dict(radius="x"),
                                 dict(radius=1, outer=2), dict(radius2=(1, 2))])
def test_a_bad_radius_is_refused_before_any_device_call(bad):
    import gcn_grabcut as g
    with pytest.raises(ValueError):
        g.ModifyMask("grow", **bad)
    for fn in (g.grow_mask, g.shrink_mask, g.open_mask, g.close_mask):
        kw = {k: v for k, v in bad.items() if k != "outer"}
        if kw != bad:
            continue
        with pytest.raises(ValueError):
            fn(M, **kw)


def test_two_radius_steps_and_ops():
    import gcn_grabcut as g
    for bad in (dict(inner=-1), dict(inner=1, outer=-2), dict(inner=1, outer=float("nan")), dict(inner=1, radius2=3),
                dict(inner=None), dict(outer=2), dict(radius2=(1, -1)), dict(radius2=(1, 2), outer=1), dict(inner=40000)):
        for fn in (g.border_mask, g.mask_to_trimap):
            with pytest.raises(ValueError):
                fn(M, **bad)
    for op in ("dilate", 6, -1, None):
        with pytest.raises(ValueError, match="op must be"):
            g.ModifyMask(op, 1)
    with pytest.raises(ValueError, match="ModifyMask"):
        g.modify_mask(M, ("grow", 1))


def test_shapes_and_max_distance_are_checked_first():
    import gcn_grabcut as g
    with pytest.raises(ValueError, match="must be \\(H, W\\)"):
        g.mask_distance(np.zeros((2, 3, 4), np.uint8))
    with pytest.raises(ValueError, match="must be \\(H, W\\)"):
        g.grow_mask(np.zeros(5, np.uint8), 1)
    with pytest.raises(ValueError, match="must be \\(B, H, W\\)"):
        g.mask_distance_batch(M)
    with pytest.raises(ValueError, match="must be \\(B, H, W\\)"):
        g.modify_mask_batch(M, g.ModifyMask("grow", 1))
    with pytest.raises(ValueError, match="empty masks"):
        g.mask_distance_batch(np.zeros((2, 0, 3), np.uint8))
    for bad in (dict(max_distance=-1), dict(max_distance=float("nan")), dict(max_distance=1, max_distance2=1),
                dict(max_distance2=-4), dict(max_distance=30000)):
        with pytest.raises(ValueError):
            g.mask_distance(M, **bad)
    assert g.mask_distance_batch(np.zeros((0, 4, 4), np.uint8)).shape == (0, 4, 4)
    assert g.modify_mask_batch(np.zeros((0, 4, 4), np.uint8), g.ModifyMask("grow", 1)).shape == (0, 4, 4)
    m = np.array([[0, 3], [1, 0]], np.uint8)
    assert np.array_equal(g.modify_mask(m), m != 0)                                     # no step: the mask, normalised
    d = g.mask_distance(m, max_distance=0.5)                                            # below every distance: no device call
    assert np.array_equal(d, np.where(m != 0, -np.inf, np.inf))
    assert np.array_equal(g.mask_distance(m, squared=True, signed=False, max_distance2=0), np.full((2, 2), 2 ** 31 - 1))


def test_result_methods_are_methods_and_refuse_a_missing_full_result():
    from gcn_grabcut import ModifyMask, SegmentationResult
    z = np.zeros((2, 2), np.uint8)
    r = SegmentationResult(image=np.zeros((2, 2, 3), np.uint8), binary_mask=z, trimap=z, segments=z.astype(np.int32),
                           overlay=np.zeros((2, 2, 3), np.uint8), rgba=np.zeros((2, 2, 4), np.uint8))
    with pytest.raises(ValueError, match="full"):
        r.modified(ModifyMask("grow", 1), full=True)
    with pytest.raises(ValueError, match="full"):
        r.trimap_from_mask(1, full=True)
    with pytest.raises(ValueError):
        r.trimap_from_mask(-1)
    assert not {"modified", "trimap_from_mask"} & {f.name for f in dataclasses.fields(SegmentationResult)}


def test_exports_header_section_and_signatures():
    import gcn_grabcut as g
    from gcn_grabcut import _native
    for name in ("ModifyMask", "mask_distance", "mask_distance_batch", "modify_mask", "modify_mask_batch", "grow_mask",
                 "shrink_mask", "open_mask", "close_mask", "border_mask", "mask_to_trimap"):
        assert name in g.__all__ and hasattr(g, name)
    header = (ROOT / "include" / "ggc.h").read_text()
    k2 = header[header.index("/* K2"):header.index("int ggc_mask_distance")]
    for phrase in ("DISTANCE", "BORDER", "FAR", "CAP", "never 0", "GGC_DIST_BORDER_BG", "GGC_E_SHAPE", "GGC_E_INVALID_ARG",
                   "2 bytes per pixel", "No host synchronisation"):
        assert phrase in k2, phrase
    k3 = header[header.index("/* K3"):header.index("int ggc_modify_mask")]
    for phrase in ("GROW", "SHRINK", "BORDER", "OPEN", "CLOSE", "TRIMAP", "may alias", "no host round trip"):
        assert phrase in k3, phrase
    assert header.index("/* K1") < header.index("/* K2") < header.index("/* K3") < header.index("/* O0")
    assert len(_native.SIGNATURES["ggc_mask_distance"]) == 9 and len(_native.SIGNATURES["ggc_modify_mask"]) == 11
    assert int(re.search(r"#define GGC_VERSION (\d+)", header).group(1)) >= 409


def test_command_lines_parse_the_new_options():
    import inference
    import matte
    p = inference.build_parser()
    a = p.parse_args(["--image", "x.png", "--modify", "shrink:2", "--modify", "trimap:1.5:4", "--save", "mask", "modified"])
    assert [s.args() for s in a.modify] == [(1, 4, 0, False), (5, 2, 16, False)] and "modified" in a.save
    assert p.parse_args(["--image", "x.png"]).modify == []
    for bad in ("shrink", "shrink:-1", "melt:2", "grow:1:2", "grow:x", "border:1:2:3"):
        with pytest.raises(SystemExit):
            p.parse_args(["--image", "x.png", "--modify", bad])
    q = matte.build_parser().parse_args(["--image", "x.png", "--mask", "m.png", "--band", "3:5"])
    assert q.mask == "m.png" and q.band == "3:5" and q.trimap is None
