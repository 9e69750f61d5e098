"""experiment helper: the CPU study behind the full-resolution banded cut.

    python3 tools/full_cut_study.py [--table] [--thin]        (no flag: both)

No device is used: the numbers come from tests/full_cut_ref.py (ggc_lift_labels restated in numpy, then the CPU oracle's
convert_color8, grabcut and clean_mask, which existing tests hold bit-exact to the device entries).

  --table  synthetic_image(240, 320, 30000 + s) for s = 0..5 from the 60x80 working size (4x4 box mean); working mask =
           box mean of the truth >= 0.5, and that rolled by one working pixel to the right.  Wrong pixels against the
           truth, summed over the six scenes: the lifted mask (bilinear >= 0.5), the guided upsample >= 0.5 (r 8, eps
           1e-4, today's full.binary_mask) and the banded cut (1 iteration, seed 0, clean_mask 0.002) at bands 2, 4, 6
           (the default, ceil(1.5 ratio)) and 8
  --thin   96x128 from 24x32, seeds 30000..30003, good masks: the cut's wrong pixels per scene at bands 2, 4 and 6 (a
           component thinner than twice the band keeps no definite seed and the cut may delete it)"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "gcn-grabcut_amd"))
import full_cut_ref as fc  # noqa: E402


def table():
    bands = (2, 4, 6, 8)
    rows = fc.study_totals(bands)
    print("full-size mask | good working mask | shifted working mask")
    print(f"lifted working mask (bilinear >= 0.5) | {rows['lifted'][0]} | {rows['lifted'][1]}")
    print(f"guided upsample >= 0.5 (r 8, eps 1e-4) | {rows['guided'][0]} | {rows['guided'][1]}")
    for b in bands:
        print(f"banded cut, band {b} | {rows[('cut', b)][0]} | {rows[('cut', b)][1]}")


def thin():
    print("seed | lifted | band 2 | band 4 | band 6")
    for s in range(30000, 30004):
        full, truth, _ = fc.scene(96, 128, s, 4)
        good, _ = fc.working_masks(truth, 4)
        errs = [fc.wrong(fc.chain(good, full, b), truth) for b in (2, 4, 6)]
        print(f"{s} | {fc.wrong(fc.lift_labels(good, (96, 128), 0)[1], truth)} | " + " | ".join(str(e) for e in errs))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--thin", action="store_true")
    a = ap.parse_args()
    if a.table or not a.thin:
        table()
    if a.thin or not a.table:
        thin()
