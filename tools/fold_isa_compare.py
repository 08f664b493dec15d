#!/usr/bin/env python3
"""Compile-time comparison of the fold kernels between two source trees.

For each tree, compiles the fold translation units to device assembly with the
flags of dpf-go_amd/Makefile (CXXFLAGS, restated in FLAGS below: keep them equal)
plus -Rpass-analysis=kernel-resource-usage (no GPU needed),
then prints one line per kernel instantiation: VGPRs, AGPRs, SGPR spills,
scratch, LDS, waves/SIMD, instruction count, v_readlane / v_writelane counts
(before / after) and whether the ISA text, comments stripped, is identical.
Exit status 1 if a hard condition fails: scratch or VGPR spills nonzero, AGPRs,
LDS or occupancy unequal, or VGPRs above the first tree's.

    tools/fold_isa_compare.py PARENT_TREE/dpf-go_amd dpf-go_amd [-o table.txt]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

UNITS = ["pir_fold_sliced", "pir_fold_grouped_mfma", "pir_fold_grouped"]
KERNELS = ("k_fold_mfma", "k_fold_grouped_mfma", "k_fold_grouped", "k_fold_sliced_direct")
FLAGS = "-O3 -std=c++17 -fPIC -Wall -Wno-unused-result".split()
FIELDS = {"VGPRs": "vgpr", "AGPRs": "agpr", "SGPRs Spill": "sspill", "VGPRs Spill": "vspill",
          "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occ"}


def compile_unit(tree, unit, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    s = os.path.join(out, unit + ".s")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", *FLAGS, "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join("csrc", unit + ".hip"), "-o", s],
                       cwd=tree, stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.exit(r.stderr)
    return s, r.stderr


def short_name(mangled):
    """_ZN4dpfk11k_fold_mfmaILi1ELi2E...Lb0EEEv... -> k_fold_mfma<1,2,...,0>"""
    m = re.match(r"_ZN4dpfk\d+(k_[a-z_]+?)(?:I((?:L[ib]\d+E)+)EEv|E)", mangled)
    if not m:
        return mangled
    args = re.findall(r"L[ib](\d+)E", m.group(2) or "")
    return m.group(1) + ("<%s>" % ",".join(args) if args else "")


def kernels_of(tree):
    """{mangled name: {resource figures, insts, readlane, writelane, isa}}"""
    res = {}
    with tempfile.TemporaryDirectory() as out, ThreadPoolExecutor(len(UNITS)) as ex:
        for s, remarks in ex.map(lambda u: compile_unit(tree, u, out), UNITS):
            cur = None
            for line in remarks.split("\n"):
                m = re.search(r"remark: +(.*?): (\S+) \[-Rpass", line)
                if not m:
                    continue
                if m.group(1) == "Function Name":
                    cur = res.setdefault(m.group(2), {})
                elif m.group(1) in FIELDS:
                    cur[FIELDS[m.group(1)]] = int(m.group(2))
            name, body = None, []
            for line in open(s):
                line = line.split(";")[0].rstrip()
                m = re.match(r"(_Z\w+):$", line)
                if m and m.group(1) in res:
                    name, body = m.group(1), []
                elif name and line.strip().startswith(".Lfunc_end"):
                    k = res[name]
                    k["isa"] = "\n".join(body)
                    ins = [b.split()[0] for b in body if b.startswith("\t") and not b.strip().startswith(".")]
                    k["insts"] = len(ins)
                    k["readlane"] = sum(i.startswith("v_readlane") for i in ins)
                    k["writelane"] = sum(i.startswith("v_writelane") for i in ins)
                    name = None
                elif name and line.strip():
                    body.append(line)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    A, B = kernels_of(a.before), kernels_of(a.after)
    if set(A) != set(B):
        sys.exit("the two trees instantiate different kernels: %s" % sorted(set(A) ^ set(B)))
    rows = sorted((short_name(n), n) for n in A)
    rows = [r for r in rows if r[0].split("<")[0] in KERNELS]
    cols = ["vgpr", "agpr", "sspill", "vspill", "scratch", "lds", "occ", "insts", "readlane", "writelane"]
    head = ["kernel", "VGPRs", "AGPRs", "SGPRspill", "VGPRspill", "scratch", "LDS bytes", "waves/SIMD", "insts",
            "v_readlane", "v_writelane", "ISA"]
    table, bad = [head], []
    for short, n in rows:
        x, y = A[n], B[n]
        table.append([short] + ["%d / %d" % (x[c], y[c]) for c in cols] + ["identical" if x["isa"] == y["isa"] else "differs"])
        if y["scratch"] or y["vspill"] or any(x[c] != y[c] for c in ("agpr", "lds", "occ")) or y["vgpr"] > x["vgpr"]:
            bad.append(short)
    wd = [max(len(r[i]) for r in table) for i in range(len(head))]
    text = "hipcc %s --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; before / after\n" % " ".join(FLAGS)
    text += "".join("  ".join(c.ljust(w) for c, w in zip(r, wd)).rstrip() + "\n" for r in table)
    text += "%d kernels, %d with identical ISA; hard conditions: %s\n" % (
        len(rows), sum(r[-1] == "identical" for r in table[1:]), "FAILED for " + ", ".join(bad) if bad else "all hold")
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
