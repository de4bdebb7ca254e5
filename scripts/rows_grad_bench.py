#!/usr/bin/env python
"""The backward of the fp32 row path (csrc/rows_grad.hip through HipBackend.linear_rows_grad / rowvec_grad) at the shapes
of the model, next to the torch sequence that gives the same gradients on the same GPU:
  linear_rows_grad (M, K, N) = (8, 1536, 12288) and (64, 1536, 12288), fp32 w, act_in GELU  (AOE projector.2)
  linear_rows_grad (8, 1280, 18560), fp16 w, act_in SiLU                                    (the 22 time_emb_proj)
  rowvec_grad (B, HW, C) = (8, 4096, 320), fp16                                             (a resnet's time row)
torch: a = act(x); dw = dy.T @ a; db = dy.sum(0); dx = act'(x) * (dy @ w) (fp16 w: dy.half() @ w, an fp16 GEMM); and
dy.sum(1, dtype=float32) for the row.
Time: device events on the backend's stream around ``--iters`` back-to-back calls after ``--warmup``, per call; every call
takes the next of ``--sets`` operand sets (w, dw and dy of 3 sets exceed the 256 MB Infinity Cache at the large shapes), so
that a call finds its weights in HBM, as a training step does.  The per-kernel split is the median call of ``--prof-iters``
further calls under the library's dispatch timestamps (dadd_prof_*).
Bytes: the one-read-one-write traffic of the call - w read once (with dx), dw written once, x / dy read, dx / db written;
the row: dy read once, drow written.  The per-strip partials of dx (ws, written and read once) are NOT in it: GB/s is the
compulsory bytes over the time, the share of the 8 TB/s peak follows.  flop: 4 M N K.
usage: python scripts/rows_grad_bench.py [--iters 30] [--warmup 5] [--sets 3] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from progressive_stable_diffusion_amd.backend import HipBackend  # noqa: E402

PEAK_BYTES = 8.0e12      # HBM3E, MI355X
PEAK_F32 = 157.3e12      # fp32 vector FMA


def timed_events(be, fn, warmup, iters):
    with be.ctx():
        for i in range(warmup):
            fn(i)
        be.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i)
        e1.record()
        be.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters           # us per call


def kernel_split(be, fn, prof_iters):
    be.synchronize()
    be.prof_begin()
    for i in range(prof_iters):
        fn(i)
    be.synchronize()
    rec = be.prof_end()
    per = len(rec) // prof_iters
    calls = sorted((rec[i * per:(i + 1) * per] for i in range(prof_iters)), key=lambda c: sum(r[1] for r in c))
    return calls[prof_iters // 2]


def act_and_grad(x, act_in):
    if act_in == 1:
        s = torch.sigmoid(x)
        return x * s, s * (1 + x * (1 - s))
    if act_in == 2:
        phi = torch.exp(-0.5 * x * x) * 0.3989422804014327
        Phi = 0.5 * (1 + torch.erf(x * 0.7071067811865476))
        return F.gelu(x), Phi + x * phi
    return x, None


def bench_linear(be, args, m, k, n, w_dtype, act_in, lines):
    dev = be.device
    g = torch.Generator(device="cpu").manual_seed(m + k + n)
    with be.ctx():
        x = torch.randn(m, k, generator=g).to(dev)
        sets = [dict(w=(torch.randn(n, k, generator=g) * k ** -0.5).to(dev, w_dtype), dy=torch.randn(m, n, generator=g).to(dev),
                     dw=torch.empty(n, k, device=dev), db=torch.empty(n, device=dev), dx=torch.empty(m, k, device=dev))
                for _ in range(args.sets)]
        ws = torch.empty(be.linear_rows_grad_ws_numel(m, k, n), device=dev)
    be.synchronize()

    def ours(i):
        s = sets[i % args.sets]
        be.linear_rows_grad(x, s["w"], s["dy"], dx=s["dx"], dw=s["dw"], db=s["db"], ws=ws, act_in=act_in)

    def torch_seq(i):
        s = sets[i % args.sets]
        a, da = act_and_grad(x, act_in)
        torch.mm(s["dy"].t(), a, out=s["dw"])
        torch.sum(s["dy"], 0, out=s["db"])
        dx = (s["dy"].half() @ s["w"]).float() if w_dtype == torch.float16 else s["dy"] @ s["w"]
        s["dx"].copy_(dx if da is None else dx * da)

    ours_us = timed_events(be, ours, args.warmup, args.iters)
    with be.ctx():
        split = kernel_split(be, ours, args.prof_iters)
    torch_us = timed_events(be, torch_seq, args.warmup, args.iters)
    wbytes = n * k * (2 if w_dtype == torch.float16 else 4)
    nbytes = wbytes + n * k * 4 + 2 * (m * k + m * n) * 4 + n * 4
    flop = 4.0 * m * n * k
    floor_b, floor_f = nbytes / PEAK_BYTES * 1e6, flop / PEAK_F32 * 1e6
    what = f"linear_rows_grad {m}x{k}x{n} {'fp16' if w_dtype == torch.float16 else 'fp32'} w act {act_in}"
    lines.append(f"  {what:46s} {nbytes / 1e6:8.1f} {ours_us:9.1f} {nbytes / ours_us * 1e-3:7.0f} {torch_us:9.1f} {ours_us / torch_us:7.3f}"
                 f"   floors: traffic {floor_b:.1f} us, fp32 FMA {floor_f:.1f} us -> {'traffic' if floor_b >= floor_f else 'FMA'} binds; "
                 f"ws {ws.numel() * 4 / 1e6:.1f} MB")
    for name, us, _, kb in split:
        lines.append(f"      {name + ' (dispatch timestamps)':60s} {us:9.1f} us {kb / 1e6:8.1f} MB {kb / us * 1e-3:7.0f} GB/s")


def bench_rowvec(be, args, b, hw, c, lines):
    dev = be.device
    with be.ctx():
        sets = [dict(dy=torch.randn(b, hw, c, device=dev).half(), drow=torch.empty(b, c, device=dev)) for _ in range(args.sets)]
        ws = torch.empty(be.rowvec_grad_ws_numel(b, hw, c), device=dev)
    be.synchronize()

    def ours(i):
        s = sets[i % args.sets]
        be.rowvec_grad(s["dy"], s["drow"], ws)

    def torch_seq(i):
        s = sets[i % args.sets]
        torch.sum(s["dy"], 1, dtype=torch.float32, out=s["drow"])

    ours_us = timed_events(be, ours, args.warmup, args.iters)
    with be.ctx():
        split = kernel_split(be, ours, args.prof_iters)
    torch_us = timed_events(be, torch_seq, args.warmup, args.iters)
    nbytes = b * hw * c * 2 + b * c * 4
    what = f"rowvec_grad {b}x{hw}x{c} fp16"
    lines.append(f"  {what:46s} {nbytes / 1e6:8.1f} {ours_us:9.1f} {nbytes / ours_us * 1e-3:7.0f} {torch_us:9.1f} {ours_us / torch_us:7.3f}"
                 f"   floor: traffic {nbytes / PEAK_BYTES * 1e6:.1f} us (the operand fits the caches: the launches bind)")
    for name, us, _, kb in split:
        lines.append(f"      {name + ' (dispatch timestamps)':60s} {us:9.1f} us {kb / 1e6:8.1f} MB {kb / us * 1e-3:7.0f} GB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prof-iters", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="toy shapes (rehearsals)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    be = HipBackend(torch.device("cuda:0"))
    lines = [f"# rows_grad_bench --iters {args.iters} --warmup {args.warmup} --sets {args.sets}   "
             f"({torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs)",
             f"# {'what':46s} {'MB':>8s} {'us':>9s} {'GB/s':>7s} {'torch us':>9s} {'/torch':>7s}"]
    f16, f32 = torch.float16, torch.float32
    cases = [(8, 64, 96, f32, 2), (8, 64, 96, f16, 1)] if args.small else \
        [(8, 1536, 12288, f32, 2), (64, 1536, 12288, f32, 2), (8, 1280, 18560, f16, 1)]
    for m, k, n, wt, act_in in cases:
        bench_linear(be, args, m, k, n, wt, act_in, lines)
    bench_rowvec(be, args, *((2, 64, 64) if args.small else (8, 4096, 320)), lines)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
