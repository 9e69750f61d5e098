"""The per-pixel rule of csrc/ggc_wand.h on the host: a seed's reference sums and match(p, s).

The kernels of ggc_wand.hip take every match from these two functions.  A stand-alone host program
(tests/wand_rule_main.cpp) prints them for every seed position of a small image, at every sample, against random pixels and
tolerances; each line is compared with tests/wand_ref.py.  The program is built with the host sanitizers.  No device is
needed."""
import os
import subprocess
from pathlib import Path

import numpy as np

import wand_ref as ref

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_rule_equals_the_reference(tmp_path):
    exe = tmp_path / "wand_rule"
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", str(ROOT / "tests" / "wand_rule_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[-2:] == ["ok", ""] and lines[-3] == f"{len(lines) - 4} cases", r.stdout[-400:]
    head = lines[0].split()
    h, w = int(head[1]), int(head[2])
    img = np.array(head[3:], np.int64).astype(np.uint8).reshape(h, w, 3)
    cases = [tuple(int(v) for v in line.split()) for line in lines[1:-3]]
    assert len(cases) >= 3000
    seen_seeds, seen_match = set(), set()
    for sr, sc, n, tol, pr, pc, r0, r1, r2, m in cases:
        want = ref.ref_sums(img, sr, sc, n)
        assert [r0, r1, r2] == want, (sr, sc, n)
        assert bool(m) == ref.match_one(img[pr, pc], want, tol, n), (sr, sc, n, tol, pr, pc)
        seen_seeds.add((sr, sc, n))
        seen_match.add(m)
    assert len(seen_seeds) == h * w * 3 and seen_match == {0, 1}            # every corner and border position, both answers
