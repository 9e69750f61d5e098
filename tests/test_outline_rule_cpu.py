"""The 2x2 rule of csrc/ggc_outline.h on the host: which cracks leave a corner, and which of them follows an arriving crack.

The kernels of ggc_outlines.hip take every crack and every successor from these two functions, so one wrong entry would
misroute only masks that happen to hold that block.  A stand-alone host program (tests/outline_rule_main.cpp) prints both for
all 16 blocks x 4 arrival directions x 2 connectivities; the table below is written out by hand from include/ggc.h K1 (block
bits 1 = NW, 2 = NE, 4 = SW, 8 = SE; directions 0 = E, 1 = S, 2 = W, 3 = N; -1 = none of the three candidates exists) and is
also held against tests/outlines_ref.py.  The program is built with the host sanitizers.  No device is needed."""
import os
import subprocess
from pathlib import Path

import numpy as np

import outlines_ref

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# LEAVING[block]: bit d set iff a crack leaves in direction d.
#   E: SE set, NE clear.  S: SW set, SE clear.  W: NW set, SW clear.  N: NE set, NW clear.
LEAVING = [0, 4, 8, 4, 2, 2, 10, 2, 1, 5, 8, 4, 1, 1, 8, 0]
# SUCCESSOR[connectivity][block][arrival direction]; the two differ only at the saddles, blocks 6 (NE + SW) and 9 (NW + SE)
SUCCESSOR = {
    8: [(-1, -1, -1, -1), (-1, 2, 2, 2), (3, -1, 3, 3), (-1, 2, 2, 2), (1, 1, 1, -1), (1, 1, 1, -1), (3, 1, 1, 3), (1, 1, 1, -1),
        (0, 0, -1, 0), (0, 0, 2, 2), (3, -1, 3, 3), (-1, 2, 2, 2), (0, 0, -1, 0), (0, 0, -1, 0), (3, -1, 3, 3), (-1, -1, -1, -1)],
    4: [(-1, -1, -1, -1), (-1, 2, 2, 2), (3, -1, 3, 3), (-1, 2, 2, 2), (1, 1, 1, -1), (1, 1, 1, -1), (1, 1, 3, 3), (1, 1, 1, -1),
        (0, 0, -1, 0), (0, 2, 2, 0), (3, -1, 3, 3), (-1, 2, 2, 2), (0, 0, -1, 0), (0, 0, -1, 0), (3, -1, 3, 3), (-1, -1, -1, -1)],
}


def test_the_table_restates_the_reference():
    for block in range(16):
        m = np.array([[block & 1, (block >> 1) & 1], [(block >> 2) & 1, (block >> 3) & 1]], np.uint8)
        assert LEAVING[block] == sum(int(outlines_ref.leaves(m, 1, 1, d)) << d for d in range(4))
        for conn in (4, 8):
            for d in range(4):
                tr, tc = 1 - outlines_ref.STEP[d][0], 1 - outlines_ref.STEP[d][1]      # the tail of a crack arriving at (1, 1)
                if outlines_ref.leaves(m, tr, tc, d):
                    assert outlines_ref.successor(m, tr, tc, d, conn) == (1, 1, SUCCESSOR[conn][block][d])
    assert [b for b in range(16) if SUCCESSOR[4][b] != SUCCESSOR[8][b]] == [6, 9]


def test_leaving_and_successor_match_the_table(tmp_path):
    exe = tmp_path / "outline_rule"
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", str(ROOT / "tests" / "outline_rule_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    want = [f"{block} {d} {conn} {LEAVING[block]} {SUCCESSOR[conn][block][d]}"
            for block in range(16) for d in range(4) for conn in (4, 8)]
    assert lines[:len(want)] == want
    assert lines[len(want):] == ["ok", ""]
