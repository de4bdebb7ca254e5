#!/usr/bin/env python3
"""Which kernels of a device assembly dump changed: splits two `hipcc --cuda-device-only -S` outputs of the same source at
their kernel symbols and compares the instruction streams (comments, debug lines and basic-block label numbers dropped;
the kernarg segment size of the descriptor is not part of the stream).
usage: python scripts/asm_kernel_diff.py before.s after.s"""
import re
import subprocess
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):\s", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            t = line.split(";")[0].rstrip()
            if not t or t.lstrip().startswith((".loc", ".file", ".cfi", ".p2align")):
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {n: d.replace("(anonymous namespace)::", "").split("(")[0] for n, d in zip(names, r)}


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
names = demangle(sorted(set(a) | set(b)))
same = changed = 0
for n in sorted(set(a) | set(b)):
    if n not in a:
        print(f"new      {names[n]}  ({len(b[n])} lines)")
    elif n not in b:
        print(f"removed  {names[n]}")
    elif a[n] != b[n]:
        changed += 1
        print(f"CHANGED  {names[n]}  ({len(a[n])} -> {len(b[n])} lines)")
    else:
        same += 1
print(f"{same} kernels identical, {changed} changed")
