"""The region graph built from on-chip pair tables (k_region_scan, k_topology, k_emit) against the CPU oracle, on the
smallest label maps at which it can go wrong, and byte for byte against the dense-matrix path it replaces.  Every output is
compared with np.array_equal: the change moves integer counts and an ordering, no float arithmetic.

Batches below 16 images keep the dense kernels unless GGC_GRAPH_ONCHIP=2, and the library reads that once per process: every
case therefore runs twice, in this process (the default choice) and in a child process that takes the tables at any size."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import graph_cases as gc
from test_graph_gpu import _check_image

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TRIO = (0, 20, 47)                                    # far-apart 8 x 8 blocks of a 48 x 64 map


def _same_colour(lab):
    seg = gc.blocks(48, 64, 8, 8)
    for r in TRIO:
        lab[0][seg == r] = np.array([50.0, 10.0, -10.0], np.float32)
    return lab


def _large_batch():
    kinds = [gc.bands(24, 40, 7), gc.stripes(24, 40, True), gc.blocks(24, 40, 4, 4), gc.bands(24, 40, 1), gc.blocks(24, 40, 2, 2)]
    return [kinds[i % len(kinds)] for i in range(140)]


# name -> (label maps, connectivity, k_nl, edit of the Lab image or None)
CASES = {
    # hub rows are where per-row assumptions break: one region with 35 neighbours
    "hub4": (lambda: [gc.hub()], 4, 4, None),
    "hub8": (lambda: [gc.hub()], 8, 4, None),
    # every pixel is a boundary pixel: a pair's count is the stripe's whole length, folded from runs of up to 64 lanes
    "stripes_v4": (lambda: [gc.stripes(24, 40, True)], 4, 4, None),
    "stripes_v8": (lambda: [gc.stripes(24, 40, True)], 8, 4, None),
    "stripes_h4": (lambda: [gc.stripes(24, 40, False)], 4, 4, None),
    "stripes_h8": (lambda: [gc.stripes(24, 40, False)], 8, 4, None),
    # both diagonal link forms at every corner
    "blocks2x2": (lambda: [gc.blocks(32, 32, 2, 2)], 8, 4, None),
    # N = 1 has no edge, N <= k + 1 no non-local pair, N = k + 2 is the first that has them; k = 0 and the largest k
    "n1": (lambda: [gc.bands(24, 40, 1)], 4, 4, None),
    "n2": (lambda: [gc.bands(24, 40, 2)], 4, 4, None),
    "n5": (lambda: [gc.bands(24, 40, 5)], 4, 4, None),
    "n6": (lambda: [gc.bands(24, 40, 6)], 4, 4, None),
    "n6_k0": (lambda: [gc.bands(24, 40, 6)], 4, 0, None),
    "n40_k8": (lambda: [gc.bands(24, 40, 40)], 4, 8, None),
    # widths that are no multiple of 64, partial last blocks
    "odd37x53": (lambda: [gc.blocks(37, 53, 8, 8)], 8, 4, None),
    "odd65x129": (lambda: [gc.blocks(65, 129, 8, 8)], 8, 4, None),
    # different N in one batch, then the same images reversed on the same context: nothing of an earlier image or call
    # may survive in the tables
    "ragged8": (gc.ragged_batch, 8, 4, None),
    "reversed8": (lambda: gc.ragged_batch()[::-1], 8, 4, None),
    "ragged4": (gc.ragged_batch, 4, 4, None),
    # from 129 images on (256 CUs) one workgroup scans an image and stores its boxes instead of merging them
    "large_batch": (_large_batch, 8, 4, None),
    # 96 x 128 of 2 x 2 blocks: N = 3072, whose bitset alone would be over 1 MB: the dense path
    "too_many_nodes": (lambda: [gc.blocks(96, 128, 2, 2)], 4, 4, None),
    # 256 labels scattered over 64 x 96 pixels have about 17 000 distinct adjacent pairs, the table holds 6 144: the scan
    # raises its overflow word and the batch, the small image next to it included, is rebuilt through the dense matrix
    "too_many_pairs": (lambda: [gc.scattered(64, 96, 256, seed=3), gc.blocks(64, 96, 8, 8)], 8, 4, None),
    "after_overflow": (lambda: [gc.blocks(64, 96, 8, 8)], 8, 4, None),
    # three far-apart regions of one colour on a noisy background choose each other: each pair is found from both ends
    "mutual": (lambda: [gc.blocks(48, 64, 8, 8)], 4, 4, _same_colour),
}


def check_case(oracle, ctx, name):
    make, conn, k, lab_edit = CASES[name]
    segs = make()
    g, seg, lab, hsv, grad = gc.run(ctx, segs, gc.images(segs, config_id=5), conn, k, lab_edit)
    assert list(np.diff(g["node_ptr"])) == [int(s.max()) + 1 for s in segs]
    wants = [_check_image(oracle, g, i, seg[i], lab[i], hsv[i], grad[i], conn, k) for i in range(len(segs))]
    ei, n = wants[0]["edge_index"], int(segs[0].max()) + 1
    if name.startswith("hub"):
        assert np.count_nonzero(ei[0] == 0) >= 35                  # the hub's row holds every block
    if name == "n1":
        assert g["edge_ptr"][-1] == 0
    if name in ("n2", "n5", "n6_k0"):
        assert wants[0]["n_edges"] == 2 * (n - 1)                  # the chain of bands and nothing else
    if name == "n6":
        assert wants[0]["n_edges"] > 2 * (n - 1)
    if name == "too_many_pairs":
        assert wants[0]["n_edges"] > 2 * 6144
    if name == "mutual":
        for a in TRIO:
            for b in TRIO:
                if a < b:
                    assert np.count_nonzero((ei[0] == a) & (ei[1] == b)) == 1
    return g


@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_oracle(oracle, gpu_ctx, name):
    check_case(oracle, gpu_ctx, name)


CHILD_SCRIPT = """
import sys
sys.path[:0] = [r'{root}', r'{root}/src', r'{root}/tests']
import graph_cases as gc
import test_graph_onchip_gpu as t
from oracle import oracle
from gcn_grabcut import _native
oracle.lib()
ctx = _native.get_context(0)
for name in t.CASES:
    print('RESULT', name, gc.digest(t.check_case(oracle, ctx, name)), flush=True)
"""


def test_every_case_on_chip_and_dense_in_child_processes(oracle, tmp_path):
    """One child takes the on-chip tables at every batch size (GGC_GRAPH_ONCHIP=2), one never (0).  Each checks every case
    against the oracle in the order above, so that the overflow cases and the calls after them share one context; then the
    two must agree on every output byte."""
    script = tmp_path / "cases.py"
    script.write_text(CHILD_SCRIPT.format(root=ROOT))
    got = {}
    for knob in ("2", "0"):
        env = dict(os.environ)
        env["GGC_GRAPH_ONCHIP"] = knob
        r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, (knob, r.stdout[-500:], r.stderr[-2000:])
        got[knob] = [x.split()[1:] for x in r.stdout.splitlines() if x.startswith("RESULT")]
        assert [x[0] for x in got[knob]] == list(CASES), (knob, r.stdout[-500:])
    assert got["2"] == got["0"]
