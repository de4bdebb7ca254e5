#!/usr/bin/env python
"""Weight / bias gradient of the UNet's 4-channel end convs (csrc/end_grad.hip, ``HipBackend.end_wgrad``) at the SD-1.x
shape at B = 8 (64 x 64 latents, Cw = 320, Ct = 4), both modes (IN: conv_in, OUT: conv_out) and both 16-bit types, beside
the same weight gradient from torch in the same run: ``torch.nn.grad.conv2d_weight`` on 16-bit GPU tensors (the thin
operand rounded beforehand, the wide one handed over as the NCHW view of the same NHWC memory; torch computes dw only, no
bias sum).  Event pairs on the backend stream, the two alternating, median over the iterations; a third column gives
the kernels' own dispatch timestamps (dadd_prof_*: the main kernel and the finish kernel of one call, summed).
GB/s counts the compulsory traffic: wide and thin read once, dw and dbias written once.  `err64` is the largest
difference of each weight gradient from the same gradient computed in float64 on the CPU from the same 16-bit operands
(the kernel accumulates in fp32 and stores fp32; torch stores the 16-bit type and accumulates its own way).
``--sweep`` adds the fp16 call over a range of splitm (the default among them), with the two kernels' dispatch times apart.
usage: python scripts/end_grad_bench.py [--iters 30] [--sweep] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from progressive_stable_diffusion_amd import lib as L  # noqa: E402
from progressive_stable_diffusion_amd.backend import HipBackend  # noqa: E402

B, H, W, CT, CW = 8, 64, 64, 4, 320


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sweep", action="store_true", help="also time the fp16 call over a range of splitm, per kernel")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    be = HipBackend(torch.device("cuda:0"))
    m = B * H * W
    lines = [f"# end_grad_bench --iters {args.iters}   B = {B}, {H} x {W}, Ct = {CT}, Cw = {CW}, M = {m}   "
             f"({torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs)",
             f"# {'mode':4s} {'type':>5s} {'splitm':>6s} | {'end_wgrad us':>12s} {'GB/s':>7s} {'kernels us':>10s} | {'torch us':>9s} "
             f"{'GB/s':>7s} | {'new/torch':>9s}  {'err64 new':>9s} {'err64 torch':>11s}"]
    g = torch.Generator().manual_seed(0)
    for dt in (torch.float16, torch.bfloat16):
        for mode, name in ((L.END_WGRAD_IN, "IN"), (L.END_WGRAD_OUT, "OUT")):
            thin = be.to_device(torch.randn(B, CT, H, W, generator=g))
            wide = be.to_device(torch.randn(B, H, W, CW, generator=g).to(dt))
            shape = (CW, 9, 8) if mode == L.END_WGRAD_IN else (CT, 9, CW)
            nb = CW if mode == L.END_WGRAD_IN else CT
            dw, db = be.empty(shape, torch.float32), be.empty((nb,), torch.float32)
            splitm = be.end_wgrad_splitm(m, CW)
            partial = be.empty((be.end_wgrad_partial_numel(splitm, CT, CW, mode),), torch.float32)
            with be.ctx():
                thin16 = thin.to(dt)
                wide_nchw = wide.permute(0, 3, 1, 2)
            ref = [None]

            def new():
                be.end_wgrad(thin, wide, dw, dbias=db, mode=mode, splitm=splitm, partial=partial)

            def torch_wgrad():
                with be.ctx():
                    if mode == L.END_WGRAD_IN:
                        ref[0] = torch.nn.grad.conv2d_weight(thin16, (CW, CT, 3, 3), wide_nchw, padding=1)
                    else:
                        ref[0] = torch.nn.grad.conv2d_weight(wide_nchw, (CT, CW, 3, 3), thin16, padding=1)

            for _ in range(3):
                new()
                torch_wgrad()
            be.synchronize()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.iters)]
            with be.ctx():
                for a, m_, z in ev:
                    a.record()
                    new()
                    m_.record()
                    torch_wgrad()
                    z.record()
            be.synchronize()
            new_us = median([a.elapsed_time(m_) * 1e3 for a, m_, _ in ev])
            old_us = median([m_.elapsed_time(z) * 1e3 for _, m_, z in ev])
            be.prof_begin()
            for _ in range(args.iters):
                new()
            rec = be.prof_end()
            per_call = len(rec) // args.iters
            kern_us = median([sum(r[1] for r in rec[i * per_call:(i + 1) * per_call]) for i in range(args.iters)])
            got = dw[:, :, :CT].permute(0, 2, 1) if mode == L.END_WGRAD_IN else dw.permute(0, 2, 1)    # [O][I][9]
            t64, w64 = thin16.double().cpu(), wide_nchw.double().cpu()
            if mode == L.END_WGRAD_IN:
                ref64 = torch.nn.grad.conv2d_weight(t64, (CW, CT, 3, 3), w64, padding=1)
            else:
                ref64 = torch.nn.grad.conv2d_weight(w64, (CT, CW, 3, 3), t64, padding=1)
            err_new = (got.reshape(ref64.shape).double().cpu() - ref64).abs().max().item()
            err_torch = (ref[0].double().cpu() - ref64).abs().max().item()
            nbytes = 2.0 * m * CW + 4.0 * m * CT + 4.0 * (dw.numel() + nb)
            lines.append(f"  {name:4s} {'f16' if dt == torch.float16 else 'bf16':>5s} {splitm:6d} | {new_us:12.1f} "
                         f"{nbytes / new_us * 1e-3:7.0f} {kern_us:10.1f} | {old_us:9.1f} {nbytes / old_us * 1e-3:7.0f} | "
                         f"{new_us / old_us:9.2f}  {err_new:9.2e} {err_torch:11.2e}")
            print(lines[-1], flush=True)
    if args.sweep:
        lines.append(f"# ---- sweep over splitm (fp16; events us per call | dispatch us of the main and the finish kernel; median of {args.iters})")
        thin = be.to_device(torch.randn(B, CT, H, W, generator=g))
        wide = be.to_device(torch.randn(B, H, W, CW, generator=g).half())
        default = be.end_wgrad_splitm(m, CW)
        for mode, name in ((L.END_WGRAD_IN, "IN"), (L.END_WGRAD_OUT, "OUT")):
            dw = be.empty((CW, 9, 8) if mode == L.END_WGRAD_IN else (CT, 9, CW), torch.float32)
            db = be.empty((CW if mode == L.END_WGRAD_IN else CT,), torch.float32)
            for splitm in sorted({1, 8, 13, 26, 52, 206, 512, default}):
                partial = be.empty((max(1, be.end_wgrad_partial_numel(splitm, CT, CW, mode)),), torch.float32)

                def call():
                    be.end_wgrad(thin, wide, dw, dbias=db, mode=mode, splitm=splitm, partial=partial)

                for _ in range(3):
                    call()
                be.synchronize()
                ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(args.iters)]
                with be.ctx():
                    for a, z in ev:
                        a.record()
                        call()
                        z.record()
                be.synchronize()
                wall = median([a.elapsed_time(z) * 1e3 for a, z in ev])
                be.prof_begin()
                for _ in range(args.iters):
                    call()
                rec = be.prof_end()
                main_us = median([r[1] for r in rec if "finish" not in r[0]])
                fin = [r[1] for r in rec if "finish" in r[0]]
                lines.append(f"#   {name:4s} splitm {splitm:4d}{' (default)' if splitm == default else '':10s} | {wall:7.1f} | "
                             f"main {main_us:7.1f}  finish {median(fin) if fin else 0.0:5.1f}")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
