#!/usr/bin/env python3
"""Compares the gfx950 ISA of two builds of a HIP object (raytracing_c_amd/csrc/rt_kernels.o), kernel by kernel: the check that a
change to shared device code (rt_dev.hip.h) left the path kernel as it was.  Needs no GPU.

    python tools/isa_compare.py parent/rt_kernels.o raytracing_c_amd/csrc/rt_kernels.o [name-filter]

Extracts the gfx950 code object of both, disassembles it, drops alignment padding after a function's end and compares the
instruction streams (mnemonics and operands; raw encodings and addresses are not printed).  Exit status 1 when a kernel both
objects have differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "llvm", "bin")


def functions(obj, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fatbin"), os.path.join(tmp, tag + ".co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + fat, "--output=" + co, "--unbundle"], check=True)
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                          capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        s = line.strip()
        m = re.match(r"^<([_A-Za-z0-9$.]+)>:$", s)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and s:
            cur.append(re.sub(r"\s*//.*$", "", s))
    for body in out.values():                      # alignment fill between functions
        while body and body[-1] in ("s_nop 0", "..."):
            body.pop()
    return out


def main():
    a_path, b_path = sys.argv[1], sys.argv[2]
    flt = sys.argv[3] if len(sys.argv) > 3 else ""
    with tempfile.TemporaryDirectory() as tmp:
        a, b = functions(a_path, tmp, "a"), functions(b_path, tmp, "b")
    differ = 0
    for k in sorted(a):
        if flt not in k:
            continue
        if k not in b:
            print("ONLY IN FIRST ", k)
        elif a[k] == b[k]:
            print("identical     ", k, len(a[k]), "instructions")
        else:
            differ += 1
            print("DIFFERENT     ", k, len(a[k]), "->", len(b[k]), "instructions")
    for k in sorted(set(b) - set(a)):
        if flt in k:
            print("ONLY IN SECOND", k, len(b[k]), "instructions")
    print(f"{differ} kernel(s) differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
