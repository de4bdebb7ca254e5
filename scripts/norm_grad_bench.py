#!/usr/bin/env python
"""Backward of GroupNorm+SiLU, LayerNorm and GEGLU (csrc/norm_grad.hip) at the shapes of a B = 4 training step of the
UNet: the resnet norms of every level (one source), the decoder's skip-concat norms (two sources), and LayerNorm /
GEGLU of the feed-forwards (tokens of 4 samples; GEGLU at F = 4 C).
Time: dispatch timestamps (dadd_prof_*), the launches of one call summed, median over the calls; the per-kernel split of
that median call follows in brackets.  GB/s: the bytes the call MUST move (x and dy read once, dx written once; h and dy
read, dh written) over that time - the kernels read x three times and dy twice for GroupNorm, so the number is the
operator's, not the memory system's.
usage: python scripts/norm_grad_bench.py [--iters 20] [--dtype f16|bf16] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from progressive_stable_diffusion_amd.backend import HipBackend  # noqa: E402

B = 4
GN_SHAPES = [  # map side, C1, C2
    (64, 320, 0), (32, 320, 0), (32, 640, 0), (16, 640, 0), (16, 1280, 0), (8, 1280, 0),
    (64, 320, 320), (64, 640, 320), (32, 640, 320), (32, 640, 640), (32, 1280, 640), (16, 1280, 640), (16, 1280, 1280),
    (8, 1280, 1280)]
FF_SHAPES = [(4096, 320), (1024, 640), (256, 1280), (64, 1280)]       # tokens per sample, C


def median_call(rec, iters):
    per = len(rec) // iters
    calls = sorted((rec[i * per:(i + 1) * per] for i in range(iters)), key=lambda c: sum(r[1] for r in c))
    mid = calls[iters // 2]
    split = " + ".join(f"{r[0].replace('_kernel', '').replace('_bf16', '')} {r[1]:.1f}" for r in mid)
    return sum(r[1] for r in mid), split


def timed(be, fn, iters):
    for _ in range(3):
        fn()
    be.synchronize()
    be.prof_begin()
    for _ in range(iters):
        fn()
    return median_call(be.prof_end(), iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtype", choices=("f16", "bf16"), default="f16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dt = torch.float16 if args.dtype == "f16" else torch.bfloat16
    be = HipBackend(torch.device("cuda:0"))
    lines = [f"# norm_grad_bench --iters {args.iters} --dtype {args.dtype}   B = {B}   ({torch.cuda.get_device_name(0)}, "
             f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs)",
             f"# {'op and shape':40s} {'MB':>8s} {'us':>8s} {'GB/s':>8s}  launches of the median call (us)"]
    g = torch.Generator().manual_seed(0)

    def rnd(*shape):
        return be.to_device(torch.randn(*shape, generator=g).to(dt))

    def row(name, nbytes, us, split):
        lines.append(f"  {name:40s} {nbytes / 1e6:8.2f} {us:8.1f} {nbytes / us * 1e-3:8.0f}  [{split}]")
        print(lines[-1], flush=True)

    for side, c1, c2 in GN_SHAPES:
        c = c1 + c2
        x1, x2, dy = rnd(B, side, side, c1), (rnd(B, side, side, c2) if c2 else None), rnd(B, side, side, c)
        gamma, beta = be.to_device(1 + 0.2 * torch.randn(c, generator=g)), be.to_device(0.2 * torch.randn(c, generator=g))
        kw = dict(dx1=be.empty(x1.shape, dt), dx2=be.empty(x2.shape, dt) if c2 else None, dgamma=be.empty((c,), torch.float32),
                  dbeta=be.empty((c,), torch.float32), groups=32, eps=1e-5, silu=True,
                  ws=be.empty((be.groupnorm_grad_ws_numel(B, side * side, c, 32),), torch.float32))
        us, split = timed(be, lambda: be.groupnorm_grad(x1, x2, dy, gamma, beta, **kw), args.iters)
        name = f"groupnorm+silu {side}x{side} C {c1}" + (f"+{c2}" if c2 else "")
        row(name, 3.0 * B * side * side * c * 2, us, split)
    for tokens, c in FF_SHAPES:
        m = B * tokens
        x, dy, gamma = rnd(m, c), rnd(m, c), be.to_device(1 + 0.2 * torch.randn(c, generator=g))
        kw = dict(dx=be.empty((m, c), dt), dgamma=be.empty((c,), torch.float32), dbeta=be.empty((c,), torch.float32),
                  ws=be.empty((be.layernorm_grad_ws_numel(m, c),), torch.float32))
        us, split = timed(be, lambda: be.layernorm_grad(x, dy, gamma, **kw), args.iters)
        row(f"layernorm {m}x{c}", 3.0 * m * c * 2, us, split)
    for tokens, c in FF_SHAPES:
        m, f = B * tokens, 4 * c
        h, dy, y, dh = rnd(m, 2 * f), rnd(m, f), be.empty((m, f), dt), be.empty((m, 2 * f), dt)
        us, split = timed(be, lambda: be.geglu(h, y), args.iters)
        row(f"geglu forward {m}x{f}", 3.0 * m * f * 2, us, split)
        us, split = timed(be, lambda: be.geglu_grad(h, dy, dh), args.iters)
        row(f"geglu backward {m}x{f}", 5.0 * m * f * 2, us, split)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
