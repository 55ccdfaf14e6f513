#!/usr/bin/env python3
"""Instruction census of the step kernels (CPU only): compiles csrc/cf_step.hip to gfx950 assembly with the flags of
contextflow_amd/build.py, demangles the kernel names and prints one row per kernel instantiation named on the command line:
counts of v_mfma*, other v_*, ds_*, buffer_* / global_*, s_nop, s_waitcnt, s_barrier, and .vgpr_count / .vgpr_spill_count /
.private_segment_fixed_size of the code object's metadata.  Classification is by those prefixes only.

usage: isa_census.py [-DNAME=VALUE ...] [--asm=FILE] [--keep=FILE] KERNEL [KERNEL ...]
  KERNEL: a substring of the demangled name without blanks and without "(anonymous namespace)::", e.g.
          "k_flow_step_small<Geo<16,16,16,1,3,0,0>,false,false,false,0>"; the word `eval` stands for the six evaluation
          instantiations of the cifar10 headline (three levels x plain / squeeze-folded).
  --asm=FILE reads an assembly file instead of compiling; --keep=FILE keeps the compiled assembly."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from contextflow_amd import build as B

EVAL = ["k_flow_step_small<Geo<16,16,16,1,3,0,0>,false,false,false,0>", "k_flow_step_small<Geo<16,16,16,1,3,0,0>,true,false,false,0>",
        "k_flow_step<Geo<32,8,8,4,6,0,0>,false,0,false,false>", "k_flow_step<Geo<32,8,8,4,6,0,0>,true,0,false,false>",
        "k_flow_step<Geo<64,4,4,8,6,0,0>,false,0,false,false>", "k_flow_step<Geo<64,4,4,8,6,0,0>,true,0,false,false>"]
COLS = ["v_mfma", "v_other", "ds", "vmem", "s_nop", "s_waitcnt", "s_barrier", "vgprs", "spill", "private"]


def assemble(defs, keep):
    src = os.path.join(B.CSRC, "cf_step.hip")
    out = keep
    if not out:
        fd, out = tempfile.mkstemp(suffix=".s")
        os.close(fd)
    cmd = ["hipcc"] + B.FLAGS + B.EXTRA_FLAGS.get("cf_step.hip", []) + defs + ["--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True)
    text = open(out).read()
    if not keep:
        os.remove(out)
    return text


def demangle(names):
    tool = next((t for t in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt") if shutil.which(t)), None)
    if tool is None:
        raise RuntimeError("no llvm-cxxfilt / c++filt found")
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    res = {}
    for m, d in zip(names, out):
        d = d.replace("(anonymous namespace)::", "").replace(" ", "")
        d = re.sub(r"^void", "", d)
        depth, end = 0, len(d)                      # cut the parameter list: the first '(' outside template brackets
        for i, c in enumerate(d):
            depth += (c == "<") - (c == ">")
            if c == "(" and depth == 0:
                end = i
                break
        res[m] = d[:end]
    return res


def census(text):
    """{mangled kernel name: {column: count}}"""
    rows, cur = {}, None
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    for line in text.split("\n"):
        s = line.strip()
        m = re.match(r"(\S+):", s)
        if m and m.group(1) in kernels:
            cur = rows.setdefault(m.group(1), dict.fromkeys(COLS, 0))
            continue
        if s.startswith(".amdhsa_kernel") or s.startswith(".end_amdhsa_kernel") or s.startswith(".section"):
            cur = None
            continue
        if cur is None or not s or s[0] in ".;":
            continue
        op = s.split()[0]
        if op.startswith("v_mfma"):
            cur["v_mfma"] += 1
        elif op.startswith("v_"):
            cur["v_other"] += 1
        elif op.startswith("ds_"):
            cur["ds"] += 1
        elif op.startswith("buffer_") or op.startswith("global_"):
            cur["vmem"] += 1
        elif op == "s_nop":
            cur["s_nop"] += 1
        elif op == "s_waitcnt":
            cur["s_waitcnt"] += 1
        elif op == "s_barrier":
            cur["s_barrier"] += 1
    for entry in re.split(r"^  - \.", text[text.find("amdhsa.kernels:"):], flags=re.M)[1:]:      # metadata: one YAML entry per kernel
        f = dict(re.findall(r"^    \.(name|vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s*(\S+)", entry, re.M))
        if f.get("name") in rows:
            r = rows[f["name"]]
            r["vgprs"], r["spill"], r["private"] = int(f["vgpr_count"]), int(f["vgpr_spill_count"]), int(f["private_segment_fixed_size"])
    return rows


def table(rows, names, wanted):
    lines = ["| kernel | " + " | ".join(COLS) + " | v_other + s_nop |", "|---|" + "---|" * (len(COLS) + 1)]
    for w in wanted:
        hits = [m for m in rows if w in names[m]]
        if not hits:
            raise SystemExit("no kernel matches %r" % w)
        for m in sorted(hits, key=lambda m: names[m]):
            r = rows[m]
            lines.append("| `%s` | " % names[m] + " | ".join(str(r[c]) for c in COLS) + " | %d |" % (r["v_other"] + r["s_nop"]))
    return "\n".join(lines)


def main(argv):
    defs = [a for a in argv if a.startswith("-D")]
    asm = next((a[len("--asm="):] for a in argv if a.startswith("--asm=")), None)
    keep = next((a[len("--keep="):] for a in argv if a.startswith("--keep=")), None)
    wanted = []
    for a in argv:
        if not a.startswith("-"):
            wanted += EVAL if a == "eval" else [a.replace(" ", "")]
    if not wanted:
        raise SystemExit(__doc__)
    text = open(asm).read() if asm else assemble(defs, keep)
    rows = census(text)
    print(table(rows, demangle(list(rows)), wanted))


if __name__ == "__main__":
    main(sys.argv[1:])
