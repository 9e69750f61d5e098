"""kernel_isa_diff.py OLD_CSRC NEW_CSRC: is the device code of two csrc trees the same, kernel by kernel?  CPU only.

Every *.hip of both directories is compiled to gfx950 assembly with the Makefile's flags plus --cuda-device-only -S; the
output is split per function symbol (whichever unit it sits in), comments and assembler directives other than the kernel
descriptor's .amdhsa_* lines are dropped, and .LBB<f>_<n> labels, which carry the function's index in its unit, are
renumbered by first appearance.  One line per symbol: SAME / DIFF / ONLY-OLD / ONLY-NEW, the length of its stream, its
name; the exit status is 0 only if every line says SAME."""
import collections
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -w".split()   # Makefile: CXXFLAGS


def functions(asm: str) -> dict:
    """symbol -> normalised instruction stream (+ the .amdhsa_* lines of a kernel)"""
    body, cur, desc = collections.defaultdict(list), None, None
    is_func = set(re.findall(r"^\s*\.type\s+(\S+),@function", asm, re.M))
    for raw in asm.splitlines():
        line = raw.split(";")[0].strip()
        if not line:
            continue
        if line.startswith(".amdhsa_kernel"):
            desc = line.split()[1]
        elif line == ".end_amdhsa_kernel":
            desc = None
        elif desc:
            body[desc].append(line)
        elif line.endswith(":") and line[:-1] in is_func:
            cur = line[:-1]
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur and (not line.startswith(".") or line.startswith(".LBB")):
            body[cur].append(line)
    out = {}
    for sym, lines in body.items():
        names = {}
        out[sym] = re.sub(r"\.LBB\d+_\d+", lambda m: names.setdefault(m.group(0), f".L{len(names)}"), "\n".join(lines))
    return out


def tree(csrc: Path, tmp: Path) -> dict:
    def assemble(src):
        out = tmp / (src.stem + ".s")
        subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", str(src), "-o", str(out)], check=True)
        return out.read_text()
    with concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        asms = list(pool.map(assemble, sorted(csrc.glob("*.hip"))))
    found = collections.defaultdict(list)              # a symbol may be defined in several units: compare them as a set
    for asm in asms:
        for sym, text in functions(asm).items():
            found[sym].append(text)
    return {sym: sorted(v) for sym, v in found.items()}


def main() -> int:
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        old, new = tree(Path(sys.argv[1]), Path(a)), tree(Path(sys.argv[2]), Path(b))
    syms = sorted(set(old) | set(new))
    nice = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.splitlines()
    count = collections.Counter()
    for sym, name in zip(syms, nice if len(nice) == len(syms) else syms):
        verdict = "ONLY-NEW" if sym not in old else "ONLY-OLD" if sym not in new else "SAME" if old[sym] == new[sym] else "DIFF"
        count[verdict] += 1
        print(f"{verdict:8s} {len(''.join(old.get(sym) or new[sym]).splitlines()):6d}  {name}")
    print("total: " + ", ".join(f"{v} {k}" for k, v in sorted(count.items())))
    return 0 if set(count) == {"SAME"} else 1


if __name__ == "__main__":
    sys.exit(main())
