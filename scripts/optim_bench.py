#!/usr/bin/env python
"""One optimizer step (csrc/optim.hip through optim.FusedAdamW) with EMA, 16-bit working copy and gradient zeroing on an
arena of the full model's size - weights.unet_shapes() plus the ordinal embedder, the image projection and the feature
purifier, in the reference's four parameter groups - next to the torch sequence that does the same on the same tensors:
clip_grad_norm_(foreach=True), AdamW(fused=True), torch._foreach_lerp_ for the EMA, one flat cast and one flat zero_.
Time: device events around ``--iters`` back-to-back steps after ``--warmup``, per step; the per-kernel split of the fused
step comes from a further ``--prof-iters`` steps under the library's dispatch timestamps (dadd_prof_*), median call.
Bytes: what a step MUST move per parameter (padding included: the kernels run over it) - grad_stats reads g (4 B);
the step reads p, g, m, v, ema (20 B) and writes p, m, v, ema, p16, g (22 B).  GB/s is those bytes over the time.
The torch sequence is timed without a loss scale (no unscale_ pass, no overflow check and none of their host syncs): it is
the lower bound of what torch would do.
usage: python scripts/optim_bench.py [--iters 20] [--warmup 3] [--dtype bf16|f16] [--scale 1.0] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from progressive_stable_diffusion_amd import optim as O  # noqa: E402
from progressive_stable_diffusion_amd import weights as W  # noqa: E402
from progressive_stable_diffusion_amd.backend import HipBackend  # noqa: E402


def timed_events(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters           # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prof-iters", type=int, default=5)
    ap.add_argument("--dtype", choices=("f16", "bf16"), default="bf16")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the model's tensors to take (rehearsals)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dt = torch.float16 if args.dtype == "f16" else torch.bfloat16
    dev = torch.device("cuda:0")
    be = HipBackend(dev)

    shapes = dict(W.unet_shapes())
    shapes.update(W.conditioning_shapes())
    keys = list(shapes)
    if args.scale < 1.0:
        keys = keys[::max(1, int(round(1.0 / args.scale)))]
    groups = O.reference_param_groups(keys, 1e-4, weight_decay=1e-3)
    torch.manual_seed(0)
    tensors = {k: torch.randn(shapes[k], device=dev) * 0.05 for g in groups for k in g["params"]}
    arena = O.arena_from_groups(tensors, groups, device=dev, working_dtype=dt, ema=True)
    del tensors
    fused = O.FusedAdamW(be, arena, groups, max_grad_norm=1.0, ema_decay=0.999)
    n, n_param = arena.numel, sum(arena.shapes[k].numel() for k in arena.names)
    arena.g.normal_().mul_(1e-3)
    g_keep = arena.g.clone()

    def refill():                                     # zero_grad empties g: give every step a gradient again
        arena.g.copy_(g_keep)

    refill_us = timed_events(refill, args.warmup, args.iters)

    def fused_step():
        refill()
        fused.step(update_ema=True, zero_grad=True)

    fused_us = timed_events(fused_step, args.warmup, args.iters) - refill_us
    torch.cuda.synchronize()
    be.prof_begin()
    for _ in range(args.prof_iters):
        fused.launch(update_ema=True, zero_grad=True)
    rec = be.prof_end()
    per = len(rec) // args.prof_iters
    calls = sorted((rec[i * per:(i + 1) * per] for i in range(args.prof_iters)), key=lambda c: sum(r[1] for r in c))
    mid = calls[args.prof_iters // 2]

    # the torch sequence on the same tensors
    params = [torch.nn.Parameter(arena.param(k)) for k in arena.names]
    for q, k in zip(params, arena.names):
        q.grad = arena.grad(k)
    idx, pgroups = 0, []
    for g, names in zip(groups, arena.group_names):
        pgroups.append({"params": params[idx:idx + len(names)], "lr": g["lr"], "weight_decay": g["weight_decay"]})
        idx += len(names)
    opt = torch.optim.AdamW(pgroups, betas=(0.9, 0.999), eps=1e-8, fused=True)
    emas = [arena.ema_param(k) for k in arena.names]
    datas = [q.data for q in params]

    def torch_step():
        refill()
        torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=True)
        opt.step()
        torch._foreach_lerp_(emas, datas, 1.0 - 0.999)
        arena.p16.copy_(arena.p)
        arena.g.zero_()

    torch_us = timed_events(torch_step, args.warmup, args.iters) - refill_us

    stats_b, step_b = 4.0 * n, 42.0 * n
    lines = [f"# optim_bench --iters {args.iters} --warmup {args.warmup} --dtype {args.dtype} --scale {args.scale}   "
             f"({torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs)",
             f"# {len(arena.names)} tensors, {n_param} parameters in {arena.n_groups} groups "
             f"{[len(x) for x in arena.group_names]}, arena {n} elements = {arena.n_chunks} chunks of {O.CHUNK}",
             f"# {'what':44s} {'MB':>10s} {'us':>10s} {'GB/s':>8s}",
             f"  {'fused step (3 launches, device events)':44s} {(stats_b + step_b) / 1e6:10.1f} {fused_us:10.1f} "
             f"{(stats_b + step_b) / fused_us * 1e-3:8.0f}"]
    for name, us, _, nbytes in mid:
        lines.append(f"    {name + ' (dispatch timestamps)':42s} {nbytes / 1e6:10.1f} {us:10.1f} {nbytes / us * 1e-3:8.0f}")
    lines += [f"  {'torch: clip + AdamW(fused) + lerp + cast + zero_':44s} {'':>10s} {torch_us:10.1f}",
              f"  fused / torch = {fused_us / torch_us:.3f}   (refill of g between steps, {refill_us:.1f} us, subtracted from both)"]
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
