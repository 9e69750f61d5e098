"""cg_list_tiles (csrc/ggc_cg.h) on the host: the tile list of the closed-form matte and foreground solves.

The function turns the per-tile counts of unknown pixels into the list of tiles to work on, each image's run of it, the
tile-to-slot map and the number of images to solve.  A stand-alone host program (tests/cg_tiles_main.cpp) compares it with
the brute-force "some tile with U lies within the ring" on 1x1, 1x4 and 3x3 grids, for ring 0 and ring 1, with U in every
single tile in turn, and on batches of three whose middle image has no U or is all U (skipped or not), built with the host
sanitizers.  No device is needed: the program calls no HIP function."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_tile_list_matches_brute_force(tmp_path):
    exe = tmp_path / "cg_tiles"
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", str(ROOT / "tests" / "cg_tiles_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    # per ring and grid of nt tiles: 2 nt one-image cases, the empty image and 3 batches of three, nt tiles per image each
    tiles = sum(nt * (2 * nt + 1 + 3 * 3) for nt in (1, 4, 9))
    assert r.stdout.strip() == f"ok {2 * tiles}"
