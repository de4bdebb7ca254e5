#!/usr/bin/env python
"""Fingerprint of the recorded operator lists of the engine's plans, built on the CPU with the test backend.

For every case one line per recorded op: the callable's name, every tensor argument as (buffer number in order of first
appearance of its storage, storage offset, shape, strides, dtype) and every other argument by value; then the sha256 of
that listing.  The buffer numbers make the pool's reuse part of the fingerprint, so two builders that record the same
launches on the same buffers in the same order, and only those, give the same hashes: run it on two commits and compare.
It reads nothing but ``plan.ops``.

    python scripts/plan_fingerprint.py [--case SUBSTRING ...] [--dump DIR]
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

def listing(plan):
    bufs = {}

    def show(v):
        if isinstance(v, torch.Tensor):
            n = bufs.setdefault(v.untyped_storage().data_ptr(), len(bufs))
            return f"T(buf={n}, off={v.storage_offset()}, shape={tuple(v.shape)}, strides={tuple(v.stride())}, {v.dtype})"
        if isinstance(v, (tuple, list)):
            return "(" + ", ".join(show(e) for e in v) + ")"
        return repr(v)
    lines = []
    for fn, a, k in plan.ops:
        args = [show(v) for v in a] + [f"{name}={show(k[name])}" for name in sorted(k)]
        lines.append(f"{getattr(fn, '__name__', repr(fn))}({', '.join(args)})")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", default=[], help="only the cases whose name contains this (repeatable)")
    ap.add_argument("--dump", default=None, help="directory that receives the full listing of every case")
    a = ap.parse_args()
    from progressive_stable_diffusion_amd import engine as E
    from tests.plan_cases import cases, policy, state_dicts
    from tests.torch_backend import TorchRefBackend
    unet_sd, enc_sd = state_dicts()
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
    for name, pol, build in cases(E, TorchRefBackend, unet_sd, enc_sd):
        if a.case and not any(c in name for c in a.case):
            continue
        with policy(E, pol):
            plans = build()
        for i, plan in enumerate(plans):
            lines = listing(plan)
            tag = name if len(plans) == 1 else f"{name}[{i}]"
            if a.dump:
                with open(os.path.join(a.dump, tag + ".txt"), "w") as f:
                    f.write("\n".join(lines) + "\n")
            print(f"{tag:52s} {len(lines):4d} ops  {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}", flush=True)
        del plans


if __name__ == "__main__":
    main()
