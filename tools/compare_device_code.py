#!/usr/bin/env python3
"""Are the kernels of two trees the same machine code?  For a refactor that must not touch device code.

  python tools/compare_device_code.py OLD_TREE NEW_TREE

Compiles every csrc/*.hip of both trees with the Makefile's CXXFLAGS plus --cuda-device-only -S and compares, per kernel
symbol, the instruction lines and the .amdhsa_* directives (comments stripped, .LBB<n>_ label numbers normalised): the
set of kernels over the whole library must be the same and every kernel's stream equal.  Exit status 1 otherwise."""
import glob
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("hyperspectral_super-resolution_amd", "csrc")


def parse(text, out):
    """Appends to out[kernel] the kernel's instruction, label and .amdhsa_* lines found in one assembly file."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    cur = None
    for line in text.split("\n"):
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
        m = re.match(r"(\S+):$", line)
        if m and m.group(1) in names:
            cur = out.setdefault(m.group(1), [])
        elif line.startswith(".amdhsa_kernel "):
            cur = out.setdefault(line.split()[1], [])
        elif line == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None and line and (line.startswith((".amdhsa_", ".LBB_")) or not line.startswith(".")):
            cur.append(line)


def kernels(tree):
    csrc = os.path.join(tree, CSRC)
    flags = subprocess.run(["make", "-s", "-C", csrc, "-f", "Makefile", "-f", "-", "print-flags"], text=True, check=True,
                           input="print-flags:\n\t@echo $(HIPCC) $(CXXFLAGS)\n", stdout=subprocess.PIPE).stdout.split()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        jobs = []
        for src in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
            asm = os.path.join(tmp, os.path.basename(src) + ".s")
            jobs.append((asm, subprocess.Popen(flags + ["--cuda-device-only", "-S", src, "-o", asm], stderr=subprocess.DEVNULL)))
        for asm, job in jobs:
            if job.wait() != 0:
                sys.exit(f"compile failed: {asm}")
            parse(open(asm).read(), out)
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    diff = sorted(set(old) ^ set(new)) + sorted(k for k in set(old) & set(new) if old[k] != new[k])
    ninstr = sum(sum(1 for l in v if not l.startswith(".")) for v in new.values())
    print(f"kernels {len(old)} / {len(new)}, instructions {ninstr}, differences {len(diff)}")
    for k in diff:
        print("  differs:", k)
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
