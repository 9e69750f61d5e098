"""relax_tiles_holding (csrc/ggc_relax.h) on the host: which tiles hold a pixel in their halo.

The function lists a source's tiles for the first round of the tile relaxation, on the device for geodesic hints and on the
host for intelligent scissors.  A stand-alone host program (tests/relax_tiles_main.cpp) compares it with the brute-force
"is the pixel inside that tile's 34x34 window" for all 32x32 positions of all tiles of a 3x3 grid, built with the host
sanitizers.  No device is needed: the program calls no HIP function."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_tiles_holding_a_pixel_match_brute_force(tmp_path):
    exe = tmp_path / "relax_tiles"
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", str(ROOT / "tests" / "relax_tiles_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"ok {9 * 32 * 32 * 9}"
