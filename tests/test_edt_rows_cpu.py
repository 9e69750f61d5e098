"""The 1-D row rule of csrc/ggc_edt.h on the host: given a row of column distances g, a cap and x, the minimum of
g(x')^2 + (x - x')^2.

The row kernel of ggc_distance.hip takes every result from this one function.  A stand-alone host program
(tests/edt_rows_main.cpp) runs it over every g row of length <= 6 with entries in {0, 1, 2, 5, none}, seeded random rows up
to length 300 and the worst-case row (all none but one end), at the caps {0, 1, 4, 25, 10^4}, and compares each result with
the brute minimum.  The program is built with the host sanitizers.  No device is needed."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_row_rule_equals_the_brute_minimum(tmp_path):
    exe = tmp_path / "edt_rows"
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", str(ROOT / "tests" / "edt_rows_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[-2:] == ["ok", ""] and int(lines[-3].split()[0]) > 1_000_000, r.stdout[-400:]
