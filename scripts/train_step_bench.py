#!/usr/bin/env python
"""One training step (training.Trainer) at B = 4 with 64x64 latents: forward, backward, optimizer and re-layout times,
with prepared weights (the optimizer's 16-bit copy and the one-launch re-layout of csrc/relayout.hip) and without (a cast
and a torch re-layout per product and call), and the re-layout launch alone next to the torch helper sequence it replaces.

Method: seeded weights, a tiny CLIP tower (frozen, outside the timed question), every draw injected.  Two trainers live
in one process and ALTERNATE round by round, so both see the same clocks and the same neighbours; each phase of a step
sits between two device events on torch's current stream; reported: median over ``--rounds`` with the min .. max spread.
The re-layout comparison alternates the same way: per round ``--iters`` back-to-back launches of the kernel, then
``--iters`` passes of grad_ops.dgrad_weight / _stride2 / _ups / _cout4 over the same tensors of the same arena.
GB/s counts one read of every listed weight and one write of its re-laid copy.
usage: python scripts/train_step_bench.py [--batch 4] [--image 512] [--rounds 7] [--iters 5] [--warmup 2] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from progressive_stable_diffusion_amd import grad_ops as G  # noqa: E402
from progressive_stable_diffusion_amd import training as TR  # noqa: E402
from progressive_stable_diffusion_amd import weights as W  # noqa: E402
from progressive_stable_diffusion_amd.config import default_config  # noqa: E402
from progressive_stable_diffusion_amd.diffusion_module_ip import DiffusionModuleWithIP  # noqa: E402

TINY_CLIP = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, image_size=224,
                 patch_size=14, projection_dim=32)
PHASES = ("forward", "backward", "optimizer", "relayout")


def helper(kind, taps, w16):
    if kind == "T":
        return G.dgrad_weight(w16, taps)
    return {"S2": G.dgrad_weight_stride2, "UPS": G.dgrad_weight_ups, "COUT4": G.dgrad_weight_cout4}[kind](w16)


def step_phases(tr, batch, draws):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    ev[0].record()
    loss = tr.loss(batch, is_training=False, **draws)
    ev[1].record()
    (loss * tr.optimizer.scale()).backward()
    ev[2].record()
    tr.optimizer.step(update_ema=True, zero_grad=True)
    ev[3].record()
    if tr.relayout is not None:
        tr.relayout.refresh()
    ev[4].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]          # ms


def spread(vals, unit=""):
    return f"{statistics.median(vals):9.3f} ({min(vals):.3f} .. {max(vals):.3f}){unit}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    b, side = args.batch, args.image // 8

    shapes = dict(W.unet_shapes())
    shapes.update(W.vae_shapes())
    shapes.update(W.conditioning_shapes(clip_hidden=TINY_CLIP["hidden_size"], clip_proj=TINY_CLIP["projection_dim"]))
    shapes.update(W.clip_shapes(TINY_CLIP))
    sd = W.init_state_dict(shapes, 0, warm_start_dis=False)
    cfg = default_config(**{"dataset.image_size": args.image})
    mod = DiffusionModuleWithIP(cfg, state_dict=sd, device=dev, seed=0, batch_size=b, clip_config=TINY_CLIP)
    g = torch.Generator().manual_seed(31)
    batch = tuple(v.to(dev) for v in (torch.rand(b, 3, args.image, args.image, generator=g) * 2 - 1,
                                      torch.arange(b, dtype=torch.float32) % 4, torch.randn(b, 3, 224, 224, generator=g)))
    draws = dict(t=torch.randint(0, 1000, (b,), generator=g), noise=torch.randn(b, 4, side, side, generator=g),
                 latent_noise=torch.randn(b, 4, side, side, generator=g), drop_mask=torch.zeros(b, dtype=torch.bool))
    trainers = {"prepared": TR.Trainer(mod, 1e-5, prepared=True, init_scale=4096.0),
                "plain": TR.Trainer(mod, 1e-5, prepared=False, init_scale=4096.0)}
    del sd
    times = {k: {p: [] for p in PHASES} for k in trainers}
    for r in range(args.warmup + args.rounds):
        for name, tr in trainers.items():
            ms = step_phases(tr, batch, draws)
            if r >= args.warmup:
                for p, v in zip(PHASES, ms):
                    times[name][p].append(v)

    # the re-layout launch against the torch helper sequence, same arena, alternating
    tr = trainers["prepared"]
    rl, arena = tr.relayout, tr.arena
    views = [(kind, taps, arena.param16(name)) for name, (kind, taps) in rl.kinds.items()]
    src_elems = sum(v.numel() for _, _, v in views)
    dst_elems = sum(rl.wt(name).numel() for name in rl.kinds)
    nbytes = 2.0 * (src_elems + dst_elems)

    def torch_sequence():
        for kind, taps, v in views:
            helper(kind, taps, v)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters
    kern, seq = [], []
    for r in range(args.warmup + args.rounds):
        k, s = timed(rl.refresh), timed(torch_sequence)
        if r >= args.warmup:
            kern.append(k)
            seq.append(s)

    lines = [f"# train_step_bench --batch {b} --image {args.image} --rounds {args.rounds} --iters {args.iters} --warmup {args.warmup}"
             f"   ({torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs)",
             f"# {len(arena.names)} trained tensors, arena {arena.numel} elements; {rl.n_desc} re-laid weights, {rl.n_tiles} tiles, "
             f"{src_elems} -> {dst_elems} elements",
             "# ms per phase, median (min .. max) over the rounds; fp16, loss scale 4096, EMA every step",
             f"# {'phase':12s} {'prepared weights':>34s} {'cast + torch re-layout per call':>34s}"]
    for p in PHASES:
        lines.append(f"  {p:12s} {spread(times['prepared'][p]):>34s} {spread(times['plain'][p]):>34s}")
    tot = {k: [sum(times[k][p][i] for p in PHASES) for i in range(args.rounds)] for k in trainers}
    lines.append(f"  {'step':12s} {spread(tot['prepared']):>34s} {spread(tot['plain']):>34s}")
    lines.append(f"  prepared / plain step = {statistics.median(tot['prepared']) / statistics.median(tot['plain']):.3f}")
    lines += ["# the re-layout alone: ms per pass, median (min .. max), and GB/s of one read + one write "
              f"({nbytes / 1e9:.3f} GB)",
              f"  {'relayout_kernel (1 launch)':34s} {spread(kern)}  {nbytes / statistics.median(kern) * 1e-6:8.0f} GB/s",
              f"  {'torch helpers (' + str(len(views)) + ' tensors)':34s} {spread(seq)}  {nbytes / statistics.median(seq) * 1e-6:8.0f} GB/s",
              f"  kernel / torch = {statistics.median(kern) / statistics.median(seq):.3f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
