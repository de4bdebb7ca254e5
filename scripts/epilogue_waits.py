#!/usr/bin/env python
"""Runs on the CPU: cross-compile kernel sources to gfx950 assembly (the flags of lib.build()) and count, per kernel
function, what the length of an epilogue depends on:

  loads    vector loads with a VGPR destination (global_load_* / buffer_load_* / flat_load_*, LDS-DMA excluded)
  stores   vector stores (global_store_* / buffer_store_* / flat_store_*)
  drained  loads whose NEXT instruction is `s_waitcnt vmcnt(0)`: a load taken where it is used, under a run-time
           test.  On gfx9 that wait also covers the previous store's acknowledgement, so a chain of them is a chain of
           dependent round trips.

The counts are sums over all run-time paths of a function.

    python scripts/epilogue_waits.py                       # igemm_dma, conv_halo, igemm
    python scripts/epilogue_waits.py tf_head ffn_block attn2_fused
    python scripts/epilogue_waits.py --asm some.s          # count an assembly file that already exists
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "progressive-stable-diffusion_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
DEFAULT = ("igemm_dma", "conv_halo", "igemm")

_LOAD = re.compile(r"^\s+(global|buffer|flat)_load_\w+\s")
_STORE = re.compile(r"^\s+(global|buffer|flat)_store_\w+\s")
_INSTR = re.compile(r"^\s+[a-z]\w*")          # an instruction line (labels and directives start in column 0 or with '.')
_DRAIN = re.compile(r"^\s+s_waitcnt\s.*vmcnt\(0\)")


def compile_asm(name, out):
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form=1",
                    "--cuda-device-only", "-S", os.path.join(CSRC, name + ".hip"), "-o", out],
                   check=True, capture_output=True, timeout=900)
    with open(out) as f:
        return f.read()


def functions(asm_text):
    """{mangled kernel name: instruction lines} of every kernel (.amdhsa_kernel) in the text."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm_text, flags=re.M))
    cur, body, out = None, [], {}
    for line in asm_text.splitlines():
        m = re.match(r"^(\S+):", line)
        if m and m.group(1) in kernels:
            cur, body = m.group(1), []
        elif line.startswith(".Lfunc_end") and cur:
            out[cur], cur = body, None
        elif cur and _INSTR.match(line) and not line.lstrip().startswith("."):
            body.append(line)
    return out


def count(body):
    loads = stores = drained = 0
    for k, line in enumerate(body):
        if _STORE.match(line):
            stores += 1
        elif _LOAD.match(line) and " lds" not in line.split(";")[0]:
            loads += 1
            if k + 1 < len(body) and _DRAIN.match(body[k + 1]):
                drained += 1
    return loads, stores, drained


def demangle(names):
    for tool in ("c++filt", "llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        except (OSError, subprocess.CalledProcessError):
            continue
        if len(out) == len(names):
            return dict(zip(names, out))
    return {n: n for n in names}


def table(asm_text):
    funcs = functions(asm_text)
    pretty = demangle(sorted(funcs))
    rows = []
    for name in sorted(funcs, key=lambda n: pretty[n]):
        short = re.sub(r"\(anonymous namespace\)::|dadd_bf16::|void |\(IgemmArgs( const)?(, int)?\)", "", pretty[name])
        rows.append((short, name, *count(funcs[name])))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("sources", nargs="*", default=list(DEFAULT), help="csrc/<name>.hip to compile")
    ap.add_argument("--asm", action="append", default=[], help="count this assembly file instead of compiling")
    args = ap.parse_args()
    texts = []
    for path in args.asm:
        with open(path) as f:
            texts.append((os.path.basename(path), f.read()))
    if not args.asm:
        with tempfile.TemporaryDirectory() as tmp:
            for name in args.sources:
                texts.append((name + ".hip", compile_asm(name, os.path.join(tmp, name + ".s"))))
    for label, text in texts:
        print(f"== {label}")
        print(f"{'kernel':<78} {'loads':>6} {'stores':>6} {'drained':>7}")
        for short, _, loads, stores, drained in table(text):
            print(f"{short:<78} {loads:>6} {stores:>6} {drained:>7}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
