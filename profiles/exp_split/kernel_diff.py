#!/usr/bin/env python3
"""Per-kernel comparison of two gfx950 device objects' disassembly.

Usage: kernel_diff.py OLD.o NEW.o [name-substring ...]

The objects come from `hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC
--cuda-device-only -c`.  Every kernel (a symbol with a `.kd` descriptor) is
disassembled; addresses and encodings are dropped, branch targets and the
literals of pc-relative address arithmetic are masked.  With name substrings
only the kernels whose demangled name contains one are compared.  Prints
"N of M identical" and the names that differ or exist on one side only.
"""
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels(obj):
    with tempfile.NamedTemporaryFile(suffix=".co") as co:   # the object is an offload bundle
        run(LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + obj,
            "--output=" + co.name)
        syms = run(LLVM + "llvm-objdump", "-t", "-C", co.name)
        dis = run(LLVM + "llvm-objdump", "-d", "-C", "--no-show-raw-insn", co.name)
    names = {m.group(1) for m in re.finditer(r"(?m)^.*\.protected (.*) \(\.kd\)$", syms)}
    out, cur = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", ln)
        if m:
            cur = m.group(1) if m.group(1) in names else None
            if cur:
                out[cur] = []
            continue
        if cur is None or not ln.strip() or ln.strip() == "...":   # "...": zero padding up to the next symbol
            continue
        ins = ln.split("//")[0].strip()
        ins = re.sub(r"^(s_c?branch\S*)\s.*$", r"\1 T", ins)
        ins = re.sub(r"^(s_addc?_u32 .*, )(0x[0-9a-f]+|\d+)$", r"\1LIT", ins)
        ins = re.sub(r"<[^>]*\+0x[0-9a-f]+>", "", ins).strip()
        out[cur].append(ins)
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    pick = sys.argv[3:]
    if pick:
        old = {k: v for k, v in old.items() if any(p in k for p in pick)}
        new = {k: v for k, v in new.items() if any(p in k for p in pick)}
    both = sorted(set(old) & set(new))
    same = [k for k in both if old[k] == new[k]]
    print(f"{len(same)} of {len(both)} identical")
    for k in both:
        if old[k] != new[k]:
            print(f"  differs: {k} ({len(old[k])} -> {len(new[k])} instructions)")
    for k in sorted(set(old) - set(new)):
        print(f"  only in {sys.argv[1]}: {k}")
    for k in sorted(set(new) - set(old)):
        print(f"  only in {sys.argv[2]}: {k}")
    return 0 if len(same) == len(both) else 1


if __name__ == "__main__":
    sys.exit(main())
