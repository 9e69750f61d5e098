"""Click guidance on the host: packing per-image click lists for ggc_apply_hints, and the CLI's refusal of clicks on a folder."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_pack_hints_keeps_click_order_per_image():
    from gcn_grabcut.graph_builder import pack_hints
    hints, ptr = pack_hints([([(1, 2), (3, 4)], [(5, 6)]),
                             None,
                             ([], [(7, 8), (9, 10)]),
                             ([(11.9, -12.9)], [])])
    assert hints.dtype == np.int32 and ptr.dtype == np.int32
    assert ptr.tolist() == [0, 3, 3, 5, 6]
    assert hints.tolist() == [[1, 2, 1], [3, 4, 1], [5, 6, 0],      # foreground clicks first, then background
                              [7, 8, 0], [9, 10, 0],
                              [11, -12, 1]]                          # int(r), int(c) as encode_user_hints


def test_pack_hints_images_without_clicks_get_empty_ranges():
    from gcn_grabcut.graph_builder import pack_hints
    hints, ptr = pack_hints([None, ((), ()), ([], None), None])
    assert hints.shape == (0, 3)
    assert ptr.tolist() == [0, 0, 0, 0, 0]
    hints, ptr = pack_hints([])
    assert hints.shape == (0, 3) and ptr.tolist() == [0]


def test_pack_hints_keeps_clicks_outside_the_image():
    from gcn_grabcut.graph_builder import pack_hints
    hints, ptr = pack_hints([([(-1, 0), (10**6, 5)], [(0, -7)])])
    assert hints.tolist() == [[-1, 0, 1], [10**6, 5, 1], [0, -7, 0]]
    assert ptr.tolist() == [0, 3]


@pytest.mark.parametrize("bad", [
    [([(1, 2, 3)], [])],                   # three coordinates
    [([1, 2], [])],                        # a flat pair instead of a list of pairs
    [([(1, 2)],)],                         # an entry that is not a (fg, bg) pair
    ["ab"],
    [([(float("nan"), 2)], [])],
    [([(2**40, 0)], [])],                  # does not fit the kernel's int32
])
def test_pack_hints_rejects_bad_shapes(bad):
    from gcn_grabcut.graph_builder import pack_hints
    with pytest.raises(ValueError):
        pack_hints(bad)


def test_cli_refuses_clicks_on_a_folder(tmp_path):
    r = subprocess.run([sys.executable, str(ROOT / "inference.py"), "--input", str(tmp_path), "--fg-point", "3,4"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--image" in r.stderr


def test_cli_scales_clicks_with_the_resize():
    sys.path.insert(0, str(ROOT))
    import inference
    assert inference.scale_points([(100, 150), (299, 399), (-4, 400)], (300, 400), (150, 200)) == \
        [(50, 75), (149, 199), (-2, 200)]
