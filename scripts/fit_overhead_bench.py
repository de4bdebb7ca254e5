#!/usr/bin/env python
"""What the training RUN adds to the training step (training.Trainer.fit against the bare step sequence), and what a
checkpoint costs the run, at the configuration of scripts/train_step_bench.py: B = 4 with 64x64 latents.

Method: seeded weights, a tiny CLIP tower, draws from torch's generators (``fit`` injects none).  Two trainers over one
module live in one process and ALTERNATE round by round, so both see the same clocks and the same neighbours:
  (a) the step as it was before the run existed, written out: loss -> x scale -> backward -> FusedAdamW.step -> re-layout
      refresh -> rates; no metrics, no accumulation bookkeeping;
  (b) ``fit`` over ``--steps`` batches as one epoch: step() with the device-side metrics, flush(), set_epoch(), and
      ``pop_metrics()`` every ``--log-every`` optimizer steps (its one synchronisation); no checkpoint.
A round is ``--steps`` steps between two host synchronisations, timed on the host clock (the question is host work and
synchronisation, which device events would not see); reported: ms per step, median (min .. max) over ``--rounds``.
The requirement: (b)'s median may exceed (a)'s by no more than (a)'s own min .. max spread.

``--checkpoint-dir DIR`` adds the cost of a full-size checkpoint written to DIR (and removed again): how long
``save_checkpoint(wait=False)`` keeps torch's stream busy (two events around the call) and the host in the call, how long
the background write then takes, and the same file with ``wait=True``.  Recorded only: the disk is not ours.
usage: python scripts/fit_overhead_bench.py [--batch 4] [--image 512] [--rounds 7] [--warmup 2] [--steps 50]
       [--log-every 50] [--checkpoint-dir DIR] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from progressive_stable_diffusion_amd import training as TR  # noqa: E402
from progressive_stable_diffusion_amd import weights as W  # noqa: E402
from progressive_stable_diffusion_amd.config import default_config  # noqa: E402
from progressive_stable_diffusion_amd.diffusion_module_ip import DiffusionModuleWithIP  # noqa: E402

TINY_CLIP = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, image_size=224,
                 patch_size=14, projection_dim=32)


def bare_step(tr, batch):
    """``Trainer.step`` as it stood before accumulation and metrics."""
    loss = tr.loss(batch)
    (loss * tr.optimizer.scale()).backward()
    tr.steps += 1
    update_ema = tr.steps >= tr.ema_start and tr.steps % tr.ema_every == 0
    tr.optimizer.step(update_ema=update_ema, zero_grad=True)
    tr.relayout.refresh()
    tr.set_epoch(tr.epoch)
    return loss.detach()


def spread(vals, unit=""):
    return f"{statistics.median(vals):9.3f} ({min(vals):.3f} .. {max(vals):.3f}){unit}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--log-every", type=int, default=50)
    ap.add_argument("--checkpoint-dir", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    b = args.batch

    shapes = dict(W.unet_shapes())
    shapes.update(W.vae_shapes())
    shapes.update(W.conditioning_shapes(clip_hidden=TINY_CLIP["hidden_size"], clip_proj=TINY_CLIP["projection_dim"]))
    shapes.update(W.clip_shapes(TINY_CLIP))
    sd = W.init_state_dict(shapes, 0, warm_start_dis=False)
    cfg = default_config(**{"dataset.image_size": args.image, "model.cfg_drop_prob": 0.1})
    mod = DiffusionModuleWithIP(cfg, state_dict=sd, device=dev, seed=0, batch_size=b, clip_config=TINY_CLIP)
    g = torch.Generator().manual_seed(31)
    batch = tuple(v.to(dev) for v in (torch.rand(b, 3, args.image, args.image, generator=g) * 2 - 1,
                                      torch.arange(b, dtype=torch.float32) % 4, torch.randn(b, 3, 224, 224, generator=g)))
    batches = [batch] * args.steps
    bare, run = TR.Trainer(mod, 1e-5, init_scale=4096.0), TR.Trainer(mod, 1e-5, init_scale=4096.0)
    del sd
    torch.manual_seed(0)
    times = {"bare": [], "fit": []}
    logged = []
    for r in range(args.warmup + args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for bt in batches:
            bare_step(bare, bt)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        logged += run.fit(batches, epochs=run.next_epoch + 1, log_every=args.log_every)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if r >= args.warmup:
            times["bare"].append((t1 - t0) * 1e3 / args.steps)
            times["fit"].append((t2 - t1) * 1e3 / args.steps)

    ma, mb = statistics.median(times["bare"]), statistics.median(times["fit"])
    room = max(times["bare"]) - min(times["bare"])
    lines = [f"# fit_overhead_bench --batch {b} --image {args.image} --rounds {args.rounds} --warmup {args.warmup} --steps {args.steps} "
             f"--log-every {args.log_every}   ({torch.cuda.get_device_name(0)}, "
             f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs)",
             "# ms per step on the host clock, a round = --steps steps between two synchronisations; median (min .. max) over "
             "the rounds; fp16, loss scale 4096",
             f"  (a) bare step sequence            {spread(times['bare'])}",
             f"  (b) fit, metrics, log every {args.log_every:<4d}  {spread(times['fit'])}",
             f"  (b) - (a) medians = {mb - ma:+.3f} ms; (a)'s own spread = {room:.3f} ms; within it: {mb - ma <= room}",
             "  (b) - (a) round by round: " + " ".join(f"{y - x:+.2f}" for x, y in zip(times["bare"], times["fit"]))
             + f"; median {statistics.median([y - x for x, y in zip(times['bare'], times['fit'])]):+.3f} ms",
             f"  fit logged {len(logged)} times over {run.steps} optimizer steps; last: loss {logged[-1]['loss']:.4f}, "
             f"skipped steps {sum(m['skipped_steps'] for m in logged)}" if logged else "  fit logged nothing"]

    if args.checkpoint_dir:
        os.makedirs(args.checkpoint_dir, exist_ok=True)
        path = os.path.join(args.checkpoint_dir, "fit_overhead_bench.ckpt")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        run.save_checkpoint(path, wait=False)
        e1.record()
        t1 = time.perf_counter()
        for bt in batches[:5]:                  # the run goes on while the file is written
            run.step(bt)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        run.close()
        t3 = time.perf_counter()
        size = os.path.getsize(path)
        os.remove(path)
        t4 = time.perf_counter()
        run.save_checkpoint(path, wait=True)
        t5 = time.perf_counter()
        os.remove(path)
        lines += [f"# one checkpoint, all three parts, {size / 1e9:.2f} GB, written to {args.checkpoint_dir} (recorded only: the disk "
                  "is not ours)",
                  f"  save_checkpoint(wait=False): torch's stream busy {e0.elapsed_time(e1):9.1f} ms, host in the call "
                  f"{(t1 - t0) * 1e3:9.1f} ms",
                  f"     5 steps issued meanwhile took {(t2 - t1) * 1e3:9.1f} ms ({(t2 - t1) * 200:.1f} ms per step); the file was "
                  f"complete {(t3 - t0):.1f} s after the call began",
                  f"  save_checkpoint(wait=True):  the run stands still for {(t5 - t4):9.1f} s"]
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
