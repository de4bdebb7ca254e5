#!/usr/bin/env python3
"""Handing trained weights to live plans, three ways (MI355X, full UNet, bench configuration: B = 4, 64x64 latents, fp16,
fusions on):
  (a) one ``optim.PlanRefresh.refresh()`` (csrc/plan_refresh.hip), with the bytes it reads and writes;
  (b) the same packers restated with torch ops on the device, from the same arena: what a user could write without the
      kernel (``engine``'s packers run on device views of the masters and copied into the plan's tensors);
  (c) the route without either: ``export_state_dict()`` + ``DiffusionModuleWithIP(state_dict=...)`` + first plan build +
      re-capture of the sampler graph (once: it takes seconds);
and the 50-step sampler pass before and after a ``sync_module`` on the same box.

Each timed figure is the median over ``--rounds`` rounds of ``--reps`` back-to-back calls between two events, after a
warm-up round.

usage: python scripts/plan_refresh_bench.py [--rounds 7] [--reps 5] [--skip-parent-route] > profiles/r20_a_plan_refresh_bench.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from progressive_stable_diffusion_amd import engine as E                      # noqa: E402
from progressive_stable_diffusion_amd import inference_pipeline_ip as PIPE   # noqa: E402
from progressive_stable_diffusion_amd import training as TR                  # noqa: E402
from progressive_stable_diffusion_amd import weights as W                    # noqa: E402
from progressive_stable_diffusion_amd.config import default_config           # noqa: E402
from progressive_stable_diffusion_amd.diffusion_module_ip import DiffusionModuleWithIP   # noqa: E402

DEV = torch.device("cuda:0")
TINY_CLIP = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, image_size=224,
                 patch_size=14, projection_dim=32)
GATES = {"anatomy": (0.1, 0.9), "disease": (0.9, 0.1), "both": (0.5, 0.5)}


def timed(fn, rounds, reps):
    """median, min, max in ms of one call of ``fn`` (events on torch's current stream around ``reps`` calls)."""
    out = []
    for r in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        if r:
            out.append(a.elapsed_time(b) / reps)
    return statistics.median(out), min(out), max(out)


def torch_route(arena, recipes, which):
    """(b): every recipe through the packer of ``engine`` it restates, on device views of the arena."""
    view = arena.ema_param if which == "ema" else arena.param

    def src(s):
        return view(s) if isinstance(s, str) else view(s[0])[s[1]:s[2]]
    seen = set()
    with torch.device(DEV), torch.no_grad():
        for r in recipes:
            if r.dst[0].data_ptr() in seen:
                continue
            seen.add(r.dst[0].data_ptr())
            d = r.dst
            if r.kind == "copy32":
                d[0].view(-1).copy_(torch.cat([src(s).reshape(-1) for s in r.src]))
            elif r.kind == "cast":
                d[0].view(-1).copy_(torch.cat([src(s).reshape(-1) for s in r.src]))
            elif r.kind == "cast_cin8":
                w = src(r.src[0])
                d[0].view(w.shape[0], 9, 8).zero_()
                d[0].view(w.shape[0], 9, 8)[:, :, :w.shape[1] // 9].copy_(w.view(w.shape[0], 9, -1))
            elif r.kind == "geglu":
                wf, bf = E.geglu_interleave(src(r.src[0]), src(r.src[1]))
                d[0].copy_(wf)
                d[1].copy_(bf)
            elif r.kind == "lnfold":
                ws, bs, gamma, beta = r.src
                w = torch.cat([src(s) for s in ws])
                b = torch.cat([src(s) for s in bs]) if bs else None
                w16, c1, bias = E.fold_layernorm(w, b, src(gamma), src(beta), d[0].dtype)
                if r.geglu:
                    idx = E.geglu_interleave(torch.arange(w16.shape[0])[:, None].float(), torch.zeros(w16.shape[0]))[0][:, 0].long()
                    w16, c1, bias = w16[idx], c1[idx], bias[idx]
                d[0].copy_(w16)
                d[1].copy_(c1)
                d[2].copy_(bias)
            elif r.kind == "upsfold":
                d[0].copy_(E.fold_ups_weight(src(r.src[0]).to(d[0].dtype)))
            elif r.kind == "head_stream":
                d[0].copy_(E.pack_head_stream(*[src(s) for s in r.src]))
            elif r.kind == "ffn_stream":
                st, b1p = E.pack_ffn_stream(*[src(s) for s in r.src])
                d[0].copy_(st)
                d[1].copy_(b1p)
            else:
                raise ValueError(r.kind)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3, help="timed 50-step sampler passes before and after the sync")
    ap.add_argument("--skip-parent-route", action="store_true")
    a = ap.parse_args()
    shapes = dict(W.unet_shapes())
    shapes.update(W.vae_shapes())
    shapes.update(W.conditioning_shapes(clip_hidden=TINY_CLIP["hidden_size"], clip_proj=TINY_CLIP["projection_dim"]))
    shapes.update(W.clip_shapes(TINY_CLIP))
    sd = W.init_state_dict(shapes, 0, gates=GATES, warm_start_dis=False)
    cfg = default_config(**{"dataset.image_size": 512})
    mod = DiffusionModuleWithIP(cfg, state_dict=sd, device=DEV, seed=0, batch_size=4, clip_config=TINY_CLIP)
    tr = TR.Trainer(mod, 1e-4, init_scale=4096.0)
    print(f"# {torch.cuda.get_device_name(0)}; B = 4, 64x64 latents, {mod.operand_dtype}; arena {tr.arena.numel / 1e6:.1f} M parameters")

    target, source = torch.tensor([3.0, 1.0, 2.0, 0.0], device=DEV), torch.tensor([0.0, 2.0, 1.0, 3.0], device=DEV)
    pix = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(DEV)
    lat = torch.randn(4, 4, 64, 64, generator=torch.Generator().manual_seed(2))

    def one_pass(module=mod):
        with torch.no_grad():
            return PIPE._ddim_sample_ip(module, target, source, pix, 50, DEV, steer_scale=3.0, latents=lat)

    def passes():
        one_pass()
        torch.cuda.synchronize()
        out = []
        for _ in range(a.passes):
            t0 = time.perf_counter()
            one_pass()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out
    before = passes()
    tr.sync_module("ema")
    torch.cuda.synchronize()
    after = passes()
    print(f"50-step pass, ms: before the first sync {[f'{x:.1f}' for x in before]} (median {statistics.median(before):.1f}), "
          f"after {[f'{x:.1f}' for x in after]} (median {statistics.median(after):.1f})")

    owners, _, pr = tr._refresher
    n_items = {str(dt): len(v) for dt, v in pr.items.items()}
    moved = pr.bytes_read + pr.bytes_written
    med, lo, hi = timed(lambda: pr.refresh("ema"), a.rounds, a.reps)
    print(f"(a) PlanRefresh.refresh: {pr.n_launches} launch(es), descriptors {n_items}, reads {pr.bytes_read / 1e9:.3f} GB, "
          f"writes {pr.bytes_written / 1e9:.3f} GB: {med:.3f} ms ({lo:.3f} .. {hi:.3f}) = {moved / med / 1e9:.2f} TB/s")
    recipes = [r for o in owners for r in o.recipes]
    med_b, lo_b, hi_b = timed(lambda: torch_route(tr.arena, recipes, "ema"), max(2, a.rounds // 2), 1)
    print(f"(b) the packers as torch ops on the device, {len(recipes)} recipes: {med_b:.1f} ms ({lo_b:.1f} .. {hi_b:.1f}) = "
          f"{med_b / med:.0f} x (a)")
    tr.sync_module("ema")           # (b) wrote the same values; leave the plans as the kernel writes them
    torch.cuda.synchronize()
    if not a.skip_parent_route:
        t0 = time.perf_counter()
        sd2 = tr.export_state_dict(ema=True)
        t1 = time.perf_counter()
        mod2 = DiffusionModuleWithIP(cfg, state_dict=sd2, device=DEV, seed=0, batch_size=4, clip_config=TINY_CLIP)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        one_pass(mod2)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        print(f"(c) without either: export_state_dict {t1 - t0:.2f} s + module and first plan {t2 - t1:.2f} s + first pass with "
              f"capture {t3 - t2:.2f} s = {t3 - t0:.2f} s")


if __name__ == "__main__":
    main()
