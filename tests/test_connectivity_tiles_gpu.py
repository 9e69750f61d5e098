"""The tile-local first round of ggc_slic_enforce_connectivity (k_cn_tile, k_cn_border, k_cn_finish, k_cn_flag, k_cn_rank,
k_cn_replay, k_cn_label) against the CPU oracle, pixel for pixel and count for count, on maps built around what
the tiles change: shapes at the tile edges, components that only close in another tile, small components whose replay order
decides where they go, the capacity of the on-chip queue, batches, and 40 fuzz cases.  Every call also asserts, through the
profiler scopes, the path that tests/test_connectivity_cases_cpu.py counted for it without device code.  One test runs the
hand-made cases in two child processes, with the tiles and with GGC_SLIC_CN_TILES=0, and compares digests.

The min_size = 5000 maps of tests/test_connectivity_small_gpu.py have no component above 256 pixels, and the library decides
per root what the queue cannot hold: they stay on chip.  A single-label map of their shape spills."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import connectivity_cases as cc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KNOB_ON = os.environ.get("GGC_SLIC_CN_TILES", "1") != "0"


def enforce(ctx, raw, mn, mx):
    """-> labels, counts, {scope: launches}"""
    from gcn_grabcut import _native
    raw = np.ascontiguousarray(raw, dtype=np.int32)
    b, h, w = raw.shape
    d = torch.as_tensor(raw).cuda()
    out = torch.empty(b, h, w, dtype=torch.int32, device="cuda")
    n = torch.empty(b, dtype=torch.int32, device="cuda")
    ctx.profile_enable(True)
    try:
        ctx.call("ggc_slic_enforce_connectivity", _native.current_stream(0), b, h, w, d.data_ptr(), int(mn), int(mx),
                 out.data_ptr(), n.data_ptr())
        torch.cuda.synchronize()
        ran = {s: ctx.profile_query(s)[0] for s in cc.SCOPES + ("slic_connectivity",)}
    finally:
        ctx.profile_enable(False)
    return out.cpu().numpy(), n.cpu().numpy(), ran


def check(oracle, ctx, raw, mn, mx, path=None):
    got, n, ran = enforce(ctx, raw, mn, mx)
    for i in range(raw.shape[0]):
        want, wn = oracle.slic_connectivity(raw[i], mn, mx)
        assert np.array_equal(got[i], want), (i, raw.shape, mn, mx, int((got[i] != want).sum()))
        assert n[i] == wn
    assert ran["slic_connectivity"] == 1
    for scope, must in cc.scopes_of(path or cc.expected_path(raw, mn, mx), KNOB_ON).items():
        if must is not None:
            assert (ran[scope] > 0) == must, (scope, ran, path)
    return got, n


@pytest.mark.parametrize("h", [1, cc.TH - 1, cc.TH, cc.TH + 1, 2 * cc.TH + 1])
@pytest.mark.parametrize("w", [cc.TW - 1, cc.TW, cc.TW + 1, 2 * cc.TW + 1])
def test_tile_edges(oracle, gpu_ctx, h, w):
    check(oracle, gpu_ctx, cc.noise(3, h, w, seed=100 * h + w), 6, cc.BIG, "tiles")
    one = np.full((3, h, w), 7, np.int32)
    got, n = check(oracle, gpu_ctx, one, 1, cc.BIG, "tiles")       # one kept component
    assert (got == 0).all() and (n == 1).all()
    check(oracle, gpu_ctx, one, 3, 40, "rounds")                    # all carved into pieces of 40


@pytest.mark.parametrize("name", list(cc.hand_cases()))
def test_hand_made_case(oracle, gpu_ctx, name):
    raw, mn, mx, path = cc.hand_cases()[name]
    check(oracle, gpu_ctx, raw, mn, mx, path)


@pytest.mark.parametrize("length", [cc.QCAP - 1, cc.QCAP, cc.QCAP + 1])
def test_queue_capacity(oracle, gpu_ctx, length):
    raw = cc.serpentine(48, 40, length)[None]
    got, n = check(oracle, gpu_ctx, raw, cc.QCAP + 50, cc.BIG, "spill" if length > cc.QCAP else "tiles")
    assert n[0] == 1 and (got == 0).all()                           # absorbed by the sea either way


def test_min_size_of_thousands_of_pixels(oracle, gpu_ctx):
    import test_connectivity_small_gpu as small
    check(oracle, gpu_ctx, small._noise(4, 21, 65, seed=7), 5000, cc.BIG, "tiles")
    check(oracle, gpu_ctx, small._noise(3, 200, 1, seed=8), 5000, cc.BIG, "tiles")
    check(oracle, gpu_ctx, small._speckled_blocks(3, 70, 140, seed=9), 5000, cc.BIG, "tiles")
    check(oracle, gpu_ctx, small._speckled_blocks(3, 70, 140, seed=10), 2000, 6000, "tiles")
    check(oracle, gpu_ctx, np.full((4, 21, 65), 2, np.int32), 5000, cc.BIG, "spill")     # 1365 pixels, absorbed by nothing


@pytest.mark.parametrize("k", range(40))
def test_fuzz(oracle, gpu_ctx, k):
    raw, mn, mx = cc.fuzz_case(k)
    check(oracle, gpu_ctx, raw, mn, mx, cc.FUZZ_PATHS[k])


def run_hand_cases(oracle, ctx):
    return [(name, cc.digest(*check(oracle, ctx, raw, mn, mx, path))) for name, (raw, mn, mx, path) in cc.hand_cases().items()]


CHILD_SCRIPT = """
import sys
sys.path[:0] = [r'{root}', r'{root}/src', r'{root}/tests']
import test_connectivity_tiles_gpu as t
from oracle import oracle
from gcn_grabcut import _native
oracle.lib()
for name, d in t.run_hand_cases(oracle, _native.get_context(0)):
    print('RESULT', name, d, flush=True)
"""


def test_tiles_and_rounds_agree_in_child_processes(oracle, tmp_path):
    """The knob is read once per process.  Each child checks every hand-made case against the oracle and asserts its own
    path (check reads the knob from the environment); the two must then agree on every byte."""
    script = tmp_path / "cases.py"
    script.write_text(CHILD_SCRIPT.format(root=ROOT))
    got = {}
    for knob in ("1", "0"):
        env = dict(os.environ)
        env["GGC_SLIC_CN_TILES"] = knob
        r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, (knob, r.stdout[-500:], r.stderr[-2000:])
        got[knob] = [x.split()[1:] for x in r.stdout.splitlines() if x.startswith("RESULT")]
        assert [x[0] for x in got[knob]] == list(cc.hand_cases()), (knob, r.stdout[-500:])
    assert got["1"] == got["0"]


def test_real_maps_take_the_tiles(oracle, gpu_ctx):
    """ggc_slic on four images of the bench generator at the bench shape: labels and counts equal the oracle's, the tile
    round ran and the rounds on the pending plane did not."""
    import gpu_helpers as gh
    from gcn_grabcut.synthetic import synthetic_batch
    bgr = synthetic_batch(4, 300, 400, config_id=4)
    lab = gh.preprocess(gpu_ctx, bgr)[1]
    gpu_ctx.profile_enable(True)
    try:
        seg, nn = gh.slic(gpu_ctx, lab, 600)
        torch.cuda.synchronize()
        ran = {s: gpu_ctx.profile_query(s)[0] for s in cc.SCOPES}
    finally:
        gpu_ctx.profile_enable(False)
    seg, nn, lab_h = seg.cpu().numpy(), nn.cpu().numpy(), lab.cpu().numpy()
    for i in range(4):
        want, wn = oracle.slic(lab_h[i], 600, 10.0, 1.0, True)
        assert np.array_equal(seg[i], want) and nn[i] == wn, i
    if KNOB_ON:
        assert ran["slic_cn_tiles"] == 1 and ran["slic_cn_replay"] == 1 and ran["slic_cn_rounds"] == 0 and ran["slic_cn_spill"] == 0, ran
