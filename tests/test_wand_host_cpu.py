"""The Python layer of the magic wand: Wand's validation, the packing of wand seeds through _Hints, refusals that happen
before any device call, the header's section and inference.py's new options.  No device is needed."""
import dataclasses
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_wand_validates_itself_and_maps_contiguous_to_connectivity():
    from gcn_grabcut import Wand
    assert Wand().args() == (32, 8, 1) and Wand(0, 4, True, 5).args() == (0, 4, 5)
    assert Wand(255, 8, False, 3).args() == (255, 0, 3) and Wand(contiguous=False).args() == (32, 0, 1)
    assert Wand(np.int64(7), np.int32(4), np.bool_(True), np.uint8(3)).args() == (7, 4, 3)
    with pytest.raises(dataclasses.FrozenInstanceError):
        Wand().tolerance = 3
    for bad in (dict(tolerance=-1), dict(tolerance=256), dict(tolerance=1.0), dict(tolerance=True), dict(tolerance="3"),
                dict(connectivity=0), dict(connectivity=6), dict(connectivity=True), dict(connectivity=4.0),
                dict(sample=0), dict(sample=2), dict(sample=7), dict(sample=3.0), dict(contiguous=1), dict(contiguous=None)):
        with pytest.raises(ValueError, match="Wand"):
            Wand(**bad)


def test_refusals_and_empty_calls_need_no_device():
    import gcn_grabcut as g
    img = np.zeros((4, 5, 3), np.uint8)
    assert np.array_equal(g.wand_select(img, [], []), np.zeros((4, 5), np.uint8))             # no seed: nothing selected
    sel, cnt = g.wand_select_batch(np.stack([img, img]), None, return_counts=True)
    assert sel.shape == (2, 4, 5) and not sel.any() and cnt.tolist() == [[0, 0], [0, 0]]
    assert g.wand_select_batch([], []).shape[0] == 0
    m = np.full((4, 5), 3, np.uint8)
    out = g.paint_wand(m, img)
    assert np.array_equal(out, m) and out is not m
    assert (g.paint_wand((4, 5), img) == 2).all()
    with pytest.raises(ValueError, match="does not match"):
        g.paint_wand((4, 6), img, [(0, 0)])
    with pytest.raises(ValueError, match="Wand"):
        g.wand_select(img, [(0, 0)], wand=(32, 8))
    with pytest.raises(ValueError, match="one size"):
        g.wand_select_batch([img, np.zeros((4, 6, 3), np.uint8)], [None, None])
    with pytest.raises(ValueError, match="entries"):
        g.wand_select_batch(np.stack([img, img]), [([(0, 0)], [])])
    with pytest.raises(ValueError):
        g.wand_select_batch(np.zeros((2, 4, 5, 3), np.float32), None)
    with pytest.raises(ValueError):
        g.wand_select(np.zeros((4, 5), np.uint8), [(0, 0)])


def test_hints_carry_wand_seeds_and_slice_them():
    from gcn_grabcut import Wand
    from gcn_grabcut.pipeline import _Hints
    assert _Hints.of(None, 3, 5, False, False) is None
    assert _Hints.of(None, 3, 5, False, False, wands=None, wand=Wand()) is None               # nothing given: nothing to launch
    assert _Hints.of(None, 3, 5, False, False, wands=[None, ([], []), None]) is None
    assert _Hints.of([None, ((), ()), None], 3, 5, False, False, wands=[((), ()), None, None]) is None
    h = _Hints.of(None, 4, 5, False, False, wands=[None, ([(1, 2)], [(3, 4), (0, 0)]), None, ([], [(2, 2)])], wand=Wand(9, 4))
    assert h.rows.shape == (0, 3) and h.segs is None and h.polys is None and not h.has_clicks
    assert h.wand_rows.tolist() == [[1, 2, 1], [3, 4, 0], [0, 0, 0], [2, 2, 0]] and h.wand_ptr.tolist() == [0, 0, 3, 3, 4]
    assert h.wand == Wand(9, 4) and h.wand_rows.dtype == np.int32 and h.wand_ptr.dtype == np.int32
    assert _Hints.of(None, 1, 5, False, False, wands=[([(0, 0)], [])]).wand == Wand()         # None: the defaults
    assert h.chunk(0, 1) is None and h.chunk(2, 3) is None
    c = h.chunk(1, 3)
    assert c.wand_rows.tolist() == [[1, 2, 1], [3, 4, 0], [0, 0, 0]] and c.wand_ptr.tolist() == [0, 3, 3] and c.wand == h.wand
    c = h.chunk(2, 4)
    assert c.wand_rows.tolist() == [[2, 2, 0]] and c.wand_ptr.tolist() == [0, 0, 1]
    whole = h.chunk(0, 4)
    assert np.array_equal(whole.wand_rows, h.wand_rows) and np.array_equal(whole.wand_ptr, h.wand_ptr)
    packed = _Hints.of(None, 4, 5, False, False, wands=(h.wand_rows, h.wand_ptr))             # the packed form is accepted
    assert np.array_equal(packed.wand_rows, h.wand_rows) and np.array_equal(packed.wand_ptr, h.wand_ptr)
    clicks = _Hints.of([None, ([(1, 1)], []), None, None], 4, 5, False, False, wands=[None, None, None, ([(0, 0)], [])])
    assert clicks.has_clicks and clicks.chunk(0, 2).wand_rows is None and clicks.chunk(0, 2).wand is None
    assert clicks.chunk(2, 4).wand_rows is not None and not clicks.chunk(2, 4).has_clicks
    only_clicks = _Hints.of([None, ([(1, 1)], []), None, None], 4, 5, False, False)
    assert only_clicks.wand_rows is None and only_clicks.wand is None and only_clicks.chunk(0, 4).wand_rows is None
    with pytest.raises(ValueError):
        _Hints.of(None, 3, 5, False, False, wands=[None, None])                               # wrong length
    with pytest.raises(ValueError):
        _Hints.of(None, 3, 5, False, False, wands=(h.wand_rows, h.wand_ptr))                  # packed for four images
    with pytest.raises(ValueError, match="Wand"):
        _Hints.of(None, 1, 5, False, False, wands=[([(0, 0)], [])], wand=32)


def test_exports_header_section_and_signature():
    import gcn_grabcut as g
    from gcn_grabcut import _native
    for name in ("Wand", "wand_select", "wand_select_batch", "paint_wand"):
        assert name in g.__all__ and hasattr(g, name)
    for name in ("add_wand", "run_with_wand", "wand_trimap"):
        assert hasattr(g.GrabCut, name)
    assert hasattr(g.GCNGrabCutPipeline, "segment_wand")
    header = (ROOT / "include" / "ggc.h").read_text()
    h5 = header[header.index("/* H5"):header.index("int ggc_wand_select")]
    for phrase in ("Reference colour", "Match", "Selection", "Combination", "replicated border", "GGC_E_SHAPE",
                   "GGC_E_INVALID_ARG", "no-op", "bit for bit", "GGC_WAND_SEEDS_PER_PASS", "SYNCHRONISES"):
        assert phrase in h5, phrase
    assert header.index("/* H4") < header.index("/* H5") < header.index("/* C0")
    assert header.count("GGC_WAND_SEEDS_PER_PASS") >= 2                                        # the knob table lists it
    assert len(_native.SIGNATURES["ggc_wand_select"]) == 14
    assert int(re.search(r"#define GGC_VERSION (\d+)", header).group(1)) >= 410


def test_inference_parses_the_wand_options():
    import inference
    p = inference.build_parser()
    a = p.parse_args(["--image", "x.png", "--bg-wand", "0,0 5,7", "--bg-wand", "9,9", "--fg-wand", "3,4", "--wand-tolerance", "12",
                      "--wand-connectivity", "0", "--wand-sample", "5", "--save", "selection", "mask"])
    assert a.bg_wand == [[(0, 0), (5, 7)], [(9, 9)]] and a.fg_wand == [[(3, 4)]] and "selection" in a.save
    assert inference.wand_options(p, a).args() == (12, 0, 5)
    d = p.parse_args(["--image", "x.png"])
    assert d.fg_wand == [] and d.bg_wand == [] and (d.wand_tolerance, d.wand_connectivity, d.wand_sample) == (32, 8, 1)
    assert inference.wand_options(p, d) is None
    a4 = p.parse_args(["--image", "x.png", "--fg-wand", "1,1", "--wand-connectivity", "4", "--save", "selection"])
    assert inference.wand_options(p, a4).args() == (32, 4, 1)
    assert inference.wand_options(p, p.parse_args(["--image", "x.png", "--bg-wand", "0,0"])) is not None    # seeds as hints alone
    for bad in (["--wand-connectivity", "6"], ["--wand-sample", "2"], ["--bg-wand", "1;2"], ["--fg-wand", ""]):
        with pytest.raises(SystemExit):
            p.parse_args(["--image", "x.png", *bad])
    for argv in (["--image", "x.png", "--save", "selection"],                                  # selection without seeds
                 ["--input", "dir", "--bg-wand", "0,0", "--save", "selection"],                # seeds need one image
                 ["--image", "x.png", "--bg-wand", "0,0", "--save", "selection", "--wand-tolerance", "300"]):
        with pytest.raises(SystemExit):
            inference.wand_options(p, p.parse_args(argv))
