"""The on-chip region graph (k_region_scan, k_topology, k_emit) at its table limits, 704 regions, 6144 distinct pairs and
k = 8, and at every way the scan splits an image's rows into bands.  Every image is compared with the CPU oracle by
np.array_equal, and every case also asserts which kernels ran, from the profiler scopes "graph_scan" and "graph_dense": a
silent fall-back to the dense kernels matches the oracle too.

GGC_GRAPH_ONCHIP and GGC_GRAPH_BANDS are read once per process, so all but one test run their cases in a child process,
one child per test.  The maps and what they pin are in graph_cases.py (LIMIT_CASES, fuzz_case); test_graph_cases_cpu.py
holds them to their limits without a GPU."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import graph_cases as gc
from test_graph_gpu import _check_image
from test_graph_onchip_gpu import CASES, check_case

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
# what GGC_GRAPH_ONCHIP=2 must run for the cases of test_graph_onchip_gpu.py (test_graph_cases_cpu.py counts it in numpy)
CASE_PATHS = {name: {"too_many_nodes": "dense", "too_many_pairs": "overflow"}.get(name, "onchip") for name in CASES}
ALL_PATHS = {**CASE_PATHS, **{name: c[4] for name, c in gc.LIMIT_CASES.items()}}
FUZZ_BANDS = (1, 4, 7)                                # child c runs the fuzz cases i with i % 3 == c at this band count
assert len(FUZZ_BANDS) == gc.FUZZ_PARTS


def check_maps(oracle, ctx, segs, conn, k, lab_edit=None, config_id=5):
    g, seg, lab, hsv, grad = gc.run(ctx, segs, gc.images(segs, config_id=config_id), conn, k, lab_edit)
    assert list(np.diff(g["node_ptr"])) == [int(s.max()) + 1 for s in segs]
    for i in range(len(segs)):
        _check_image(oracle, g, i, seg[i], lab[i], hsv[i], grad[i], conn, k)
    return g


def child_cases(oracle, ctx):
    """Every case in order on one context.  A case whose result differs from the oracle's is reported and the next one
    runs, so that the parent names every such case; any other error ends the child."""
    runs = [(name, lambda name=name: check_case(oracle, ctx, name)) for name in CASES]
    runs += [(name, lambda c=c: check_maps(oracle, ctx, c[0](), c[1], c[2], c[3])) for name, c in gc.LIMIT_CASES.items()]
    for name, call in runs:
        try:
            g, path = gc.traced(ctx, call)
            print("RESULT", name, gc.digest(g), path, flush=True)
        except AssertionError:
            print("RESULT", name, "differs-from-the-oracle", "-", flush=True)


def device_slic(ctx):
    def slic(bgr, n_seg):
        import gpu_helpers as gh
        seg, _ = gh.slic(ctx, gh.preprocess(ctx, bgr)[1], n_seg)
        return list(seg.cpu().numpy())
    return slic


def child_fuzz(oracle, ctx, part):
    for i in range(part, gc.FUZZ_COUNT, gc.FUZZ_PARTS):
        case = gc.fuzz_case(i)
        try:
            segs = gc.fuzz_maps(case, device_slic(ctx))
            want = gc.predict(segs, case["conn"], case["k"])          # in numpy, before the run
            _, path = gc.traced(ctx, lambda: check_maps(oracle, ctx, segs, case["conn"], case["k"], None, case["config_id"]))
        except AssertionError:
            path = "differs-from-the-oracle"
        except BaseException:
            print("FUZZ CASE FAILED", case, flush=True)
            raise
        print("RESULT", i, want, path, flush=True)
        if path != want:
            print("MISMATCH", case, flush=True)


CHILD_SCRIPT = """
import sys
sys.path[:0] = [r'{root}', r'{root}/src', r'{root}/tests']
import test_graph_onchip_limits_gpu as t
from oracle import oracle
from gcn_grabcut import _native
oracle.lib()
ctx = _native.get_context(0)
if sys.argv[1] == 'cases':
    t.child_cases(oracle, ctx)
else:
    t.child_fuzz(oracle, ctx, int(sys.argv[2]))
"""


def run_child(tmp_path, onchip, bands, *args):
    """One fresh process with the two knobs set; -> the fields of its RESULT lines."""
    script = tmp_path / "child.py"
    script.write_text(CHILD_SCRIPT.format(root=ROOT))
    env = dict(os.environ)
    env["GGC_GRAPH_ONCHIP"], env["GGC_GRAPH_BANDS"] = str(onchip), str(bands)
    r = subprocess.run([sys.executable, str(script), *map(str, args)], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, (onchip, bands, r.stdout[-1500:], r.stderr[-2000:])
    return [x.split()[1:] for x in r.stdout.splitlines() if x.startswith("RESULT")], r.stdout


@pytest.fixture(scope="module")
def dense_digests(oracle, tmp_path_factory):
    """name -> digest of every case through the dense kernels (GGC_GRAPH_ONCHIP=0), each checked against the oracle."""
    got, out = run_child(tmp_path_factory.mktemp("dense"), 0, 0, "cases")
    assert [x[0] for x in got] == list(ALL_PATHS), out[-500:]
    assert [x[0] for x in got if x[1] == "differs-from-the-oracle"] == []
    assert all(x[2] == "dense" for x in got), got
    return {x[0]: x[1] for x in got}


def test_dense_child_checks_every_case_and_never_scans(dense_digests):
    """The child that the band-count tests compare with: it stands first so that its run is this test's time."""
    assert set(dense_digests) == set(ALL_PATHS)


@pytest.mark.parametrize("bands", [1, 2, 3, 5, 8])
def test_every_case_at_a_pinned_band_count(oracle, tmp_path, dense_digests, bands):
    """All cases of test_graph_onchip_gpu.py and the limit cases, in one context and in order, with the scan's rows split
    into `bands` bands: the oracle's result for every image, the dense child's bytes, and the kernels each case must run.
    One band is how the benchmark's batch runs: there pairs6145 and one_band_overflow overflow in the scan's own insert,
    with more bands in one band's table or in k_topology's union count."""
    got, out = run_child(tmp_path, 2, bands, "cases")
    assert [x[0] for x in got] == list(ALL_PATHS), out[-500:]
    assert [x[0] for x in got if x[1] == "differs-from-the-oracle"] == []
    assert {x[0]: x[2] for x in got} == ALL_PATHS
    assert {x[0]: x[1] for x in got} == dense_digests


@pytest.mark.parametrize("part", range(len(FUZZ_BANDS)))
def test_fuzz_child(oracle, tmp_path, part):
    """A third of the 40 seeded batches (graph_cases.fuzz_case) at one band count: every image against the oracle, and the
    profiler's path equal to the one predicted in numpy from N and the distinct pairs.  Each third holds at least 10
    batches that must stay on chip, so the three hold the 30 of 40."""
    got, out = run_child(tmp_path, 2, FUZZ_BANDS[part], "fuzz", part)
    assert [int(x[0]) for x in got] == list(range(part, gc.FUZZ_COUNT, gc.FUZZ_PARTS)), out[-1500:]
    assert all(x[1] == x[2] for x in got), [x for x in out.splitlines() if x.startswith("MISMATCH")]
    assert sum(x[2] == "onchip" for x in got) >= 10, got


def test_real_superpixels_take_the_tables_by_default(oracle, gpu_ctx):
    """24 images is the smallest batch that takes the on-chip path with no knob set: device SLIC maps of synthetic
    images, every image against the oracle."""
    import gpu_helpers as gh
    from gcn_grabcut.synthetic import synthetic_batch
    assert "GGC_GRAPH_ONCHIP" not in os.environ and "GGC_GRAPH_BANDS" not in os.environ
    b, conn, k = 24, 8, 4
    _, lab, hsv, gray, grad = gh.preprocess(gpu_ctx, synthetic_batch(b, 64, 96, config_id=4))
    seg, nn = gh.slic(gpu_ctx, lab, 60)
    g, path = gc.traced(gpu_ctx, lambda: gh.graph(gpu_ctx, seg, nn, lab, hsv, grad, conn, k))
    assert path == "onchip"
    seg_h, lab_h, hsv_h, grad_h = seg.cpu().numpy(), lab.cpu().numpy(), hsv.cpu().numpy(), grad.cpu().numpy()
    assert list(np.diff(g["node_ptr"])) == [int(s.max()) + 1 for s in seg_h]
    for i in range(b):
        _check_image(oracle, g, i, seg_h[i], lab_h[i], hsv_h[i], grad_h[i], conn, k)
