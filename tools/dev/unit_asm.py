#!/usr/bin/env python3
"""Device assembly of every translation unit, to show that a reorganisation of csrc/ leaves every kernel as it was (CPU only).

usage: unit_asm.py emit DIR            compiles every csrc/*.hip with the flags of contextflow_amd/build.py plus
                                       --cuda-device-only -S into DIR/<unit>.s and replaces the per-unit symbol
                                       __hip_cuid_<hex>, a hash of the source text, with one fixed token
       unit_asm.py compare DIR_A DIR_B one line per unit: `identical` or the first differing line; exit 1 on any difference

Run `emit` in a checkout of each of the two commits (the script imports the build.py of the tree it stands in) and `compare`
the two directories.  Whole files are compared; nothing in them is classified."""
import concurrent.futures
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from contextflow_amd import build as B


def emit_one(src, out_dir):
    unit = os.path.basename(src)
    out = os.path.join(out_dir, unit[:-4] + ".s")
    cmd = ["hipcc"] + B.FLAGS + B.EXTRA_FLAGS.get(unit, []) + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr[-4000:]))
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(out).read())
    open(out, "w").write(text)
    return unit, text.count("\n")


def emit(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        for unit, lines in ex.map(lambda s: emit_one(s, out_dir), B.sources()):
            print("%-28s %7d lines" % (unit, lines))


def compare(dir_a, dir_b):
    a, b = (sorted(f for f in os.listdir(d) if f.endswith(".s")) for d in (dir_a, dir_b))
    if a != b:
        print("different units: only in %s: %s; only in %s: %s" % (dir_a, sorted(set(a) - set(b)), dir_b, sorted(set(b) - set(a))))
        return 1
    bad = 0
    for f in a:
        la, lb = (open(os.path.join(d, f)).read().split("\n") for d in (dir_a, dir_b))
        if la == lb:
            print("%-28s %7d lines  identical" % (f, len(la) - 1))
            continue
        bad += 1
        n = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
        print("%-28s DIFFERS at line %d:\n  < %s\n  > %s" % (f, n + 1, la[n] if n < len(la) else "<end>", lb[n] if n < len(lb) else "<end>"))
    print("%d of %d units identical" % (len(a) - bad, len(a)))
    return 1 if bad else 0


def main(argv):
    if len(argv) == 2 and argv[0] == "emit":
        emit(argv[1])
    elif len(argv) == 3 and argv[0] == "compare":
        sys.exit(compare(argv[1], argv[2]))
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
