#!/usr/bin/env python3
"""Compare the instruction text of kernels in two gfx950 code objects, addresses aside.

  python tools/kernel_text_diff.py A.out B.out SUBSTRING [SUBSTRING ...]

A.out / B.out: device ELFs (hipcc -save-temps leaves them as *-gfx950.out).  Every symbol whose
name holds one of the substrings is disassembled with llvm-objdump -d in both; addresses, raw
encodings and branch-target comments are dropped (a branch keeps its offset operand, so moved
code inside a kernel still shows).  Prints one line per symbol; exit status 1 if any differs.
"""
import os
import re
import subprocess
import sys

OBJDUMP = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-objdump")


def kernels(path):
    out = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout
    res, cur = {}, None
    for ln in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
        if m:
            cur = res.setdefault(m.group(1), [])
            continue
        if cur is None or not ln.strip():
            continue
        ins = ln.split("//")[0].strip()
        ins = re.sub(r"^[0-9a-f]+:\s*", "", ins)
        ins = re.sub(r"<[^>]*>", "", ins).strip()
        if ins:
            cur.append(ins)
    return res


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for sym in sorted(a):
        if not any(s in sym for s in sys.argv[3:]):
            continue
        same = sym in b and a[sym] == b[sym]
        bad += not same
        print("%-9s %6d / %6d instructions  %s" % ("identical" if same else "DIFFERENT", len(a[sym]),
                                                    len(b.get(sym, [])), sym))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
