#!/usr/bin/env python
"""Backward of attention (csrc/attn_grad.hip) at the shapes of a B = 4 training step of the UNet: attn1 (self-attention,
N = 4096 / 1024 / 256 tokens at d = 40 / 80 / 160, 8 heads, gradients written into one [B,N,3C] buffer) and one pathway
of attn2 (the same queries against 16 conditioning tokens).
Time: dispatch timestamps (dadd_prof_*), per launch (statistics, dK / dV, dQ) and summed, of the median call.  TFLOP/s:
the call's algorithmic work (2 * 9 * B * heads * Nq * Nk * d: two products in the statistics, four in dkv, three in dq)
over the summed time.
With --cond: the conditioning front-end instead (d = 96, 16 queries against 257 keys; the purifier's tail backward), each
against torch on the same tensors by events around single calls, hip and torch alternating.
usage: python scripts/attn_grad_bench.py [--iters 20] [--dtype f16|bf16] [--cond] [--out FILE]"""
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


def event_median(be, fn, warmup, iters):
    """Median over ``iters`` calls of the time between two events around ONE call on the backend stream (us): what a
    caller waits for, launch gaps between the call's kernels included."""
    with be.ctx():
        for _ in range(warmup):
            fn()
        be.synchronize()
        pairs = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            pairs.append((e0, e1))
        be.synchronize()
    times = sorted(a.elapsed_time(b) * 1e3 for a, b in pairs)
    return times[len(times) // 2], times[len(times) // 10], times[(9 * len(times)) // 10]


def cond(args):
    """--cond: the conditioning front-end's shapes.  attn_grad at the resampler shape (B 8, 8 heads, d 96, 16 queries
    against 257 keys) against torch's SDPA backward on the same fp16 tensors, and purifier_gate_tail_grad at M 128, C 768
    against its torch composition; events around single calls in one process, warm-up, median (10 % / 90 %)."""
    import torch.nn.functional as F
    be = HipBackend(torch.device("cuda:0"))
    dt = torch.float16
    g = torch.Generator().manual_seed(0)
    lines = [f"# attn_grad_bench --cond --iters {args.iters}   ({torch.cuda.get_device_name(0)}, "
             f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs)   us per call: median (10 % .. 90 %), events "
             "around one call; 'kernels' = dispatch timestamps of the median call"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def compare(name, hip_fn, torch_name, torch_fn, rounds=3):
        """hip and torch alternate, ``rounds`` times each, so that a drift of the machine shows as a spread between rounds."""
        ksum, split = timed(be, hip_fn, 20)
        say(f"  {name}: kernels {ksum:.1f} us [{split}]")
        for r in range(rounds):
            med, lo, hi = event_median(be, hip_fn, 20, args.iters)
            line = f"    round {r}: hip {med:7.1f} ({lo:.1f} .. {hi:.1f})"
            if torch_fn is not None:
                med_t, lo_t, hi_t = event_median(be, torch_fn, 20, args.iters)
                line += f"   {torch_name} {med_t:7.1f} ({lo_t:.1f} .. {hi_t:.1f})   hip / torch {med / med_t:.2f}"
            say(line)

    b, heads, d, nq, nk = 8, 8, 96, 16, 257
    c = heads * d
    q, k, v, do = (be.to_device((0.5 * torch.randn(b, n, c, generator=g)).to(dt)) for n in (nq, nk, nk, nq))
    dq, dk, dv = be.empty((b, nq, c), dt), be.empty((b, nk, c), dt), be.empty((b, nk, c), dt)
    ws = be.empty((be.attn_grad_ws_numel(b, heads, nq),), torch.float32)
    call = lambda: be.attn_grad(q, k, v, do, dq=dq, dk=dk, dv=dv, ws=ws, heads=heads)  # noqa: E731
    sdpa = None
    try:
        with be.ctx():
            qh, kh, vh = (t.view(b, -1, heads, d).transpose(1, 2).detach().requires_grad_(True) for t in (q, k, v))
            out = F.scaled_dot_product_attention(qh, kh, vh)
            doh = do.view(b, nq, heads, d).transpose(1, 2)
            torch.autograd.grad(out, (qh, kh, vh), doh, retain_graph=True)
        sdpa = lambda: torch.autograd.grad(out, (qh, kh, vh), doh, retain_graph=True)  # noqa: E731
    except Exception as e:      # (no SDPA backward for this shape in this torch build: say so, time the kernels alone)
        say(f"  torch SDPA backward not available ({type(e).__name__}: {e})")
    compare(f"attn_grad f16 B {b} heads {heads} d {d} Nq {nq} Nk {nk}", call, "torch SDPA backward", sdpa)

    m, cc = 128, 768
    img, dis, z = (be.to_device(torch.randn(m, cc, generator=g).to(dt)) for _ in range(3))
    dout, gamma, beta = be.to_device(torch.randn(m, cc, generator=g)), be.to_device(torch.ones(cc)), be.to_device(torch.zeros(cc))
    dimg, ddis, dz = (be.empty((m, cc), dt) for _ in range(3))
    dgam, dbet = be.empty((cc,), torch.float32), be.empty((cc,), torch.float32)
    ws2 = be.empty((be.purifier_gate_tail_grad_ws_numel(m, cc),), torch.float32)
    call2 = lambda: be.purifier_gate_tail_grad(img, dis, z, dout, gamma, dimg=dimg, ddis=ddis, dz=dz, dgamma=dgam,  # noqa: E731
                                               dbeta=dbet, ws=ws2)
    with be.ctx():
        u0 = img.float() - torch.sigmoid(z.float()) * dis.float()
        _, mean, rstd = torch.ops.aten.native_layer_norm(u0, [cc], gamma, beta, 1e-5)

    def torch_tail():           # sigmoid, mul, sub, native_layer_norm_backward (mean / rstd given), then the three outputs
        gt = torch.sigmoid(z.float())
        u = img.float() - gt * dis.float()
        du, _, _ = torch.ops.aten.native_layer_norm_backward(dout, u, [cc], mean, rstd, gamma, beta, [True, True, True])
        dd = -gt * du
        return du.to(dt), dd.to(dt), (dd * dis.float() * (1.0 - gt)).to(dt)
    compare(f"purifier_gate_tail_grad f16 M {m} C {cc}", call2, "torch composition", torch_tail)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtype", choices=("f16", "bf16"), default="f16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cond", action="store_true", help="the conditioning front-end's shapes against torch, by events")
    args = ap.parse_args()
    if args.cond:
        return cond(args)
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
