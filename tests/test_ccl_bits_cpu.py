"""The two lane-mask functions of csrc/ggc_ccl.h on the host: where a lane's run starts, and how long a run is.

Every labelling kernel takes a pixel's first parent and a run's length from them, so an error at a lane near 0 or 63 would
mislabel only images whose runs happen to cross that lane.  A stand-alone host program (tests/ccl_bits_main.cpp) compares both
with a plain walk over the lanes: for all pairs (start candidates, valid lanes) of a 12-bit window at lanes 0, 26 and 52 (the
last reaches lane 63), for all pairs of the all-ones, the two alternating and the 64 single-bit masks, and for 4096 seeded
random pairs.  It is built with the host sanitizers, which would report a shift by 64 or a count of zeros of 0.  No device
is needed: the program calls no HIP function."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_run_start_and_run_length_match_a_walk_over_the_lanes(tmp_path):
    exe = tmp_path / "ccl_bits"
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", str(ROOT / "tests" / "ccl_bits_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"ok {3 * 4096 * 4096 + 67 * 67 + 4096}"
