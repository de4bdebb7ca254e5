#!/usr/bin/env python
"""Backward of attention (csrc/attn_grad.hip) at the shapes of a B = 4 training step of the UNet: attn1 (self-attention,
N = 4096 / 1024 / 256 tokens at d = 40 / 80 / 160, 8 heads, gradients written into one [B,N,3C] buffer) and one pathway
of attn2 (the same queries against 16 conditioning tokens).
Time: dispatch timestamps (dadd_prof_*), per launch (statistics, dK / dV, dQ) and summed, of the median call.  TFLOP/s:
the call's algorithmic work (2 * 9 * B * heads * Nq * Nk * d: two products in the statistics, four in dkv, three in dq)
over the summed time.
usage: python scripts/attn_grad_bench.py [--iters 20] [--dtype f16|bf16] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from progressive_stable_diffusion_amd.backend import HipBackend  # noqa: E402

B, HEADS = 4, 8
SHAPES = [(4096, 40), (1024, 80), (256, 160)]        # tokens per sample, head dim


def timed(be, fn, iters):
    for _ in range(3):
        fn()
    be.synchronize()
    be.prof_begin()
    for _ in range(iters):
        fn()
    rec = be.prof_end()
    per = len(rec) // iters
    calls = sorted((rec[i * per:(i + 1) * per] for i in range(iters)), key=lambda c: sum(r[1] for r in c))
    mid = calls[iters // 2]
    return sum(r[1] for r in mid), " + ".join(f"{r[0].split('_kernel')[0].replace('attn_grad_', '')} {r[1]:.1f}" for r in mid)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtype", choices=("f16", "bf16"), default="f16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dt = torch.float16 if args.dtype == "f16" else torch.bfloat16
    be = HipBackend(torch.device("cuda:0"))
    lines = [f"# attn_grad_bench --iters {args.iters} --dtype {args.dtype}   B = {B}, {HEADS} heads   "
             f"({torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs)",
             f"# {'shape':40s} {'us':>8s} {'TFLOP/s':>8s}  launches of the median call (us)"]
    g = torch.Generator().manual_seed(0)

    def rnd(*shape):
        return be.to_device((0.5 * torch.randn(*shape, generator=g)).to(dt))

    def row(name, flop, us, split):
        lines.append(f"  {name:40s} {us:8.1f} {flop / us * 1e-6:8.1f}  [{split}]")
        print(lines[-1], flush=True)

    for n, d in SHAPES:
        c = HEADS * d
        qkv, dy, dqkv = rnd(B, n, 3 * c), rnd(B, n, c), be.empty((B, n, 3 * c), dt)
        ws = be.empty((be.attn_grad_ws_numel(B, HEADS, n),), torch.float32)
        q, k, v = (qkv[..., i * c:(i + 1) * c] for i in range(3))
        dq, dk, dv = (dqkv[..., i * c:(i + 1) * c] for i in range(3))
        us, split = timed(be, lambda: be.attn_grad(q, k, v, dy, dq=dq, dk=dk, dv=dv, ws=ws, heads=HEADS), args.iters)
        row(f"self N {n} d {d}", 18.0 * B * HEADS * n * n * d, us, split)
        kv, dkv, gate = rnd(B, 48, 4 * c), be.zeros((B, 48, 4 * c), dt), be.to_device(torch.tensor([0.8]))
        pk, pv, pdk, pdv = kv[:, 16:32, :c], kv[:, 16:32, c:2 * c], dkv[:, 16:32, :c], dkv[:, 16:32, c:2 * c]
        qc, dqc = rnd(B, n, c), be.empty((B, n, c), dt)
        us, split = timed(be, lambda: be.attn_grad(qc, pk, pv, dy, dq=dqc, dk=pdk, dv=pdv, ws=ws, heads=HEADS,
                                                   do_scale_dev=gate), args.iters)
        row(f"pathway Nq {n} Nk 16 d {d}", 18.0 * B * HEADS * n * 16 * d, us, split)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
