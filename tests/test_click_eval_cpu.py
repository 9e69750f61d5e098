"""metrics.noc_summary on hand-made IoU curves (no GPU)."""
import numpy as np
import pytest

from gcn_grabcut.metrics import noc_summary


def test_noc_summary_hand_made_curves():
    ious = np.array([
        [0.91, 0.92, 0.93, 0.94],     # reached at 0
        [0.10, 0.20, 0.30, 0.40],     # never reached
        [0.50, 0.86, 0.70, 0.95],     # 0.85 reached at 1 then lost; 0.90 reached at 3
        [0.80, 0.84, 0.85, 0.85],     # 0.85 reached exactly at 2
    ])
    s = noc_summary(ious, (0.85, 0.90), 3)
    assert s["noc"][0.85].tolist() == [0, 3, 1, 2]
    assert s["noc"][0.90].tolist() == [0, 3, 3, 3]
    assert s["nof"] == {0.85: 1, 0.90: 2}
    assert np.allclose(s["mean_iou"], ious.mean(axis=0))


def test_noc_summary_no_clicks_and_bad_shapes():
    s = noc_summary(np.array([[0.9], [0.2]]), (0.85,), 0)
    assert s["noc"][0.85].tolist() == [0, 0] and s["nof"][0.85] == 1
    with pytest.raises(ValueError):
        noc_summary(np.zeros((2, 4)), (0.85,), 5)
