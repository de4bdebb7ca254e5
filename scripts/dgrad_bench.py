#!/usr/bin/env python
"""Data gradient of the resampling convs (csrc/dgrad.hip) at the six Downsample2D / Upsample2D shapes of the SD-1.x UNet
at B = 8 (BASELINE config 4: 512 x 512 images, 64 x 64 latents), beside the composed path on the stride-1 kernels in the
same run:
  stride 2: dy zero-dilated to Hi x Wi by torch, then ``HipBackend.dgrad`` (3 of 4 gathered rows are zeros);
  upsample: ``HipBackend.dgrad`` at 2H x 2W, then the 2 x 2 sum in torch (fp32, rounded once).
Both columns: event pairs on the backend stream around the whole path (the weight re-layout is outside: a step does it
once per weight), the two paths alternating, median over the iterations.  A third column gives the new kernel's dispatch
timestamps (dadd_prof_*).  TFLOP/s counts the USEFUL work, the forward conv's 2 B Ho Wo 9 C N; peak = 2.5 PFLOP/s (dense
16-bit MFMA of the MI355X).  `max diff` is the largest difference between the two paths' dx.
usage: python scripts/dgrad_bench.py [--iters 20] [--dtype f16|bf16|both] [--out FILE]"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from progressive_stable_diffusion_amd import grad_ops  # noqa: E402
from progressive_stable_diffusion_amd import lib as L  # noqa: E402
from progressive_stable_diffusion_amd.backend import HipBackend  # noqa: E402

PEAK_TF = 2500.0
B = 8
SHAPES = [  # name, mode, Hi (input map of the forward conv), C = N
    ("down 320 @64->32", "stride2", 64, 320),
    ("down 640 @32->16", "stride2", 32, 640),
    ("down 1280 @16->8", "stride2", 16, 1280),
    ("up 1280 @8->16", "ups", 8, 1280),
    ("up 1280 @16->32", "ups", 16, 1280),
    ("up 640 @32->64", "ups", 32, 640),
]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtype", choices=("f16", "bf16", "both"), default="both")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    be = HipBackend(torch.device("cuda:0"))
    lines = [f"# dgrad_bench --iters {args.iters} --dtype {args.dtype}   B = {B}   ({torch.cuda.get_device_name(0)}, "
             f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs)",
             f"# {'shape':18s} {'type':>5s} {'grid':>9s} | {'dgrad us':>9s} {'TF/s':>7s} {'of peak':>8s} {'kernel us':>9s} | "
             f"{'composed us':>11s} {'TF/s':>7s} | {'new/composed':>12s}  max diff"]
    g = torch.Generator().manual_seed(0)
    for dt in [torch.float16, torch.bfloat16] if args.dtype == "both" else [torch.float16 if args.dtype == "f16" else torch.bfloat16]:
        for name, mode, hi, c in SHAPES:
            n, ups = c, mode == "ups"
            ho = 2 * hi if ups else hi // 2
            dy = be.to_device(torch.randn(B, ho, ho, n, generator=g).to(dt))
            w16 = be.to_device((torch.randn(n, 9 * c, generator=g) * (9 * c) ** -0.5).to(dt))
            with be.ctx():
                wt_new = grad_ops.dgrad_weight_ups(w16) if ups else grad_ops.dgrad_weight_stride2(w16)
                wt_old = grad_ops.dgrad_weight(w16, 9)
            dx_new, dx_old = be.empty((B, hi, hi, c), dt), [None]
            kw = dict(ups=1) if ups else dict(stride=2)

            def new():
                be.dgrad_resample(dy, wt_new, dx_new, **kw)

            def composed():
                with be.ctx():
                    if ups:
                        big = torch.empty((B, ho, ho, c), dtype=dt, device=be.device)
                        be.dgrad(dy, wt_old, big, taps=9)
                        dx_old[0] = big.view(B, hi, 2, hi, 2, c).float().sum((2, 4)).to(dt)
                    else:
                        dil = torch.zeros((B, hi, hi, n), dtype=dt, device=be.device)
                        dil[:, ::2, ::2] = dy
                        dx_old[0] = torch.empty((B, hi, hi, c), dtype=dt, device=be.device)
                        be.dgrad(dil, wt_old, dx_old[0], taps=9)

            for _ in range(3):
                new()
                composed()
            be.synchronize()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.iters)]
            with be.ctx():
                for a, m_, z in ev:
                    a.record()
                    new()
                    m_.record()
                    composed()
                    z.record()
            be.synchronize()
            new_us = median([a.elapsed_time(m_) * 1e3 for a, m_, _ in ev])
            old_us = median([m_.elapsed_time(z) * 1e3 for _, m_, z in ev])
            be.prof_begin()
            for _ in range(args.iters):
                new()
            rec = be.prof_end()
            kern_us = median([r[1] for r in rec])
            diff = (dx_new.float() - dx_old[0].float()).abs().max().item()
            flop = 2.0 * B * ho * ho * 9 * c * n
            d, ch = L.DgradDesc(), L.DgradChoice()       # the grid the launch decided on (host-only resolve)
            d.dy, d.wt, d.dx = dy.data_ptr(), wt_new.data_ptr(), dx_new.data_ptr()
            d.B, d.Hi, d.Wi, d.C, d.Ho, d.Wo, d.N = B, hi, hi, c, ho, ho, n
            d.mode, d.ld_dy, d.ld_dx = (L.DGRAD_UPS if ups else L.DGRAD_STRIDE2), n, c
            L.check(be.lib.dadd_conv_dgrad_resolve(ctypes.byref(d), ctypes.byref(ch)))
            lines.append(f"  {name:18s} {'f16' if dt == torch.float16 else 'bf16':>5s} {ch.grid_x:5d}x{ch.grid_y:<3d} | {new_us:9.1f} {flop / new_us * 1e-6:7.1f} "
                         f"{flop / new_us * 1e-6 / PEAK_TF:8.2%} {kern_us:9.1f} | {old_us:11.1f} {flop / old_us * 1e-6:7.1f} | "
                         f"{new_us / old_us:12.2f}  {diff:.3e}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
