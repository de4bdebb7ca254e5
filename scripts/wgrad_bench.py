#!/usr/bin/env python
"""Weight-gradient kernel (csrc/wgrad.hip) at the training shapes of BASELINE config 4 (B = 8, 512 x 512 images, 64 x 64
latents), at the backend's default splitm, beside what PyTorch-ROCm does for the same product in the same run:
``dy2d.t() @ x2d`` in the operand dtype for the linears, ``torch.nn.grad.conv2d_weight`` for the convolutions (if it runs).
HIP column: dispatch timestamps (dadd_prof_*), wgrad_kernel + wgrad_finish_kernel of one call summed, median over the
launches.  torch column: event pairs around each call, median.  TFLOP/s = 2 M N taps C / time; peak = 2.5 PFLOP/s (dense
16-bit MFMA of the MI355X).
usage: python scripts/wgrad_bench.py [--iters 20] [--dtype f16|bf16] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from progressive_stable_diffusion_amd.backend import HipBackend  # noqa: E402

PEAK_TF = 2500.0
SHAPES = [  # name, B, H, C, N, taps
    ("conv3x3 320->320 @64x64", 8, 64, 320, 320, 9),
    ("conv3x3 1280->1280 @8x8", 8, 8, 1280, 1280, 9),
    ("linear 320->2560 M=32768", 8, 64, 320, 2560, 1),
    ("linear 1280->1280 M=2048", 8, 16, 1280, 1280, 1),
]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def torch_time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return median([a.elapsed_time(b) * 1e3 for a, b in ev])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtype", choices=("f16", "bf16"), default="f16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dt = torch.float16 if args.dtype == "f16" else torch.bfloat16
    be = HipBackend(torch.device("cuda:0"))
    lines = [f"# wgrad_bench --iters {args.iters} --dtype {args.dtype}   ({torch.cuda.get_device_name(0)}, "
             f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs)",
             f"# {'shape':28s} {'splitm':>6s} {'hip us':>9s} {'TF/s':>7s} {'of peak':>8s} | {'torch us':>9s} {'TF/s':>7s} {'of peak':>8s} | "
             f"{'hip/torch':>9s}  max err/bound"]
    g = torch.Generator().manual_seed(0)
    for name, b, h, c, n, taps in SHAPES:
        m = b * h * h
        x = be.to_device(torch.randn(b, h, h, c, generator=g).to(dt))
        dy = be.to_device(torch.randn(b, h, h, n, generator=g).to(dt))
        splitm = be.wgrad_splitm(m, n, c, taps)
        dw, db = be.empty((n, taps, c), torch.float32), be.empty((n,), torch.float32)
        partial = be.empty((max(1, be.wgrad_partial_numel(splitm, n, c, taps)),), torch.float32)
        kw = dict(dbias=db, taps=taps, pad=1 if taps == 9 else 0, splitm=splitm, partial=partial)
        for _ in range(3):
            be.wgrad(dy, x, dw, **kw)
        be.synchronize()
        be.prof_begin()
        for _ in range(args.iters):
            be.wgrad(dy, x, dw, **kw)
        rec = be.prof_end()
        per_call = len(rec) // args.iters
        hip_us = median([sum(r[1] for r in rec[i * per_call:(i + 1) * per_call]) for i in range(args.iters)])
        flop = 2.0 * m * n * taps * c
        # the fp32 result against a float64 product of the same operands (one tap is enough for the convolutions)
        x2, dy2 = x.reshape(m, c), dy.reshape(m, n)
        ref, e = dy2.double().t() @ x2.double(), dy2.double().abs().t() @ x2.double().abs()
        got = dw[:, taps // 2, :].double()       # the centre tap of a 3x3: no shift, no padding
        ratio = ((got - ref).abs() / ((m + 2) * 2.0 ** -24 * e)).max().item()
        try:
            if taps == 1:
                t_us = torch_time(lambda: dy2.t() @ x2, args.iters)
            else:
                xn, dyn = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)     # channels-last NCHW views
                t_us = torch_time(lambda: torch.nn.grad.conv2d_weight(xn, (n, c, 3, 3), dyn, padding=1), args.iters)
            t_col = f"{t_us:9.1f} {flop / t_us * 1e-6:7.1f} {flop / t_us * 1e-6 / PEAK_TF:8.2%}"
            rel = f"{hip_us / t_us:9.2f}"
        except Exception as exc:  # the torch column is informative only
            t_col, rel = f"did not run: {type(exc).__name__}: {str(exc)[:60]}", "        -"
        lines.append(f"  {name:28s} {splitm:6d} {hip_us:9.1f} {flop / hip_us * 1e-6:7.1f} {flop / hip_us * 1e-6 / PEAK_TF:8.2%} | "
                     f"{t_col} | {rel}  {ratio:.3f}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
