#!/usr/bin/env python
"""Fingerprint of the recorded operator lists of the engine's plans, built on the CPU with the test backend.

For every case one line per recorded op: the callable's name, every tensor argument as (buffer number in order of first
appearance of its storage, storage offset, shape, strides, dtype) and every other argument by value; then the sha256 of
that listing.  The buffer numbers make the pool's reuse part of the fingerprint, so two builders that record the same
launches on the same buffers in the same order, and only those, give the same hashes: run it on two commits and compare.
It reads nothing but ``plan.ops``.

    python scripts/plan_fingerprint.py [--case SUBSTRING ...] [--dump DIR]
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

GATES = {"anatomy": (0.1, 0.9), "disease": (0.9, 0.1), "both": (0.5, 0.5)}
SMALL = dict(A2_MIN_TILES=1, FFN_MIN_BLOCKS=1)
POLICIES = {                     # non-default settings the tests and scripts use, each at (1, 16) fp16
    "small_tiles": SMALL,
    "small_tiles_gn_fused_0": dict(SMALL, GN_FUSED_MAX_BYTES=0),
    "ln_fold_true": dict(LN_FOLD=True),
    "ln_fold_false": dict(LN_FOLD=False),
    "no_ln_stats_from_producer": dict(LN_STATS_FROM_PRODUCER=False),
    "no_finish_gn_apply": dict(FINISH_GN_APPLY=False),
    "no_gn_in_conv": dict(GN_IN_CONV=False),
    "no_row_block_fusions": dict(FUSED_ATTN2=False, FUSED_FFN=False, FUSED_HEAD=False),
    "halo_duo": dict(HALO_DUO=True),
}


def listing(plan):
    bufs = {}

    def show(v):
        if isinstance(v, torch.Tensor):
            n = bufs.setdefault(v.untyped_storage().data_ptr(), len(bufs))
            return f"T(buf={n}, off={v.storage_offset()}, shape={tuple(v.shape)}, strides={tuple(v.stride())}, {v.dtype})"
        if isinstance(v, (tuple, list)):
            return "(" + ", ".join(show(e) for e in v) + ")"
        return repr(v)
    lines = []
    for fn, a, k in plan.ops:
        args = [show(v) for v in a] + [f"{name}={show(k[name])}" for name in sorted(k)]
        lines.append(f"{getattr(fn, '__name__', repr(fn))}({', '.join(args)})")
    return lines


def cases(E, be, unet_sd, enc_sd):
    """(name, policy overrides, builder of a list of plans)"""
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}
    for b, s in ((4, 64), (2, 32), (1, 16), (2, 8)):
        for name, d in dt.items():
            yield f"unet_{name}_b{b}_s{s}", {}, lambda b=b, s=s, d=d: [E.UNetPlan(be(), unet_sd, b, s, dtype=d)]
    yield "unet_fp16_b2_s8_no_routing_gates", {}, lambda: [E.UNetPlan(be(), unet_sd, 2, 8, use_routing_gates=False)]
    for name, pol in POLICIES.items():
        yield f"unet_fp16_b1_s16_{name}", pol, lambda: [E.UNetPlan(be(), unet_sd, 1, 16)]
    for name in ("no_ln_stats_from_producer", "no_gn_in_conv", "no_row_block_fusions"):     # (1, 16) takes none of these paths
        yield f"unet_fp16_b4_s64_{name}", POLICIES[name], lambda: [E.UNetPlan(be(), unet_sd, 4, 64)]
    yield "unet_fp16_b4_s64_weight_prefetch_2",dict(WEIGHT_PREFETCH_AHEAD=2), lambda: [E.UNetPlan(be(), unet_sd, 4, 64)]

    def shared():
        cache = {}
        return [E.UNetPlan(be(), unet_sd, 1, 16, wcache=cache), E.UNetPlan(be(), unet_sd, 2, 16, wcache=cache)]
    yield "unet_fp16_shared_wcache_b1_then_b2_s16", {}, shared
    yield "vae_decoder_b4_s64", {}, lambda: [E.VaeDecoderPlan(be(), unet_sd, 4, 64)]
    yield "vae_decoder_b1_s8", {}, lambda: [E.VaeDecoderPlan(be(), unet_sd, 1, 8)]
    yield "vae_encoder_b2_s16", {}, lambda: [E.VaeEncoderPlan(be(), enc_sd, 2, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", default=[], help="only the cases whose name contains this (repeatable)")
    ap.add_argument("--dump", default=None, help="directory that receives the full listing of every case")
    a = ap.parse_args()
    from progressive_stable_diffusion_amd import engine as E
    from progressive_stable_diffusion_amd import weights as W
    from tests.torch_backend import TorchRefBackend
    shapes = dict(W.unet_shapes())
    shapes.update(W.vae_shapes(encoder=False))
    unet_sd = W.init_state_dict(shapes, 0, gates=GATES)
    enc_sd = W.init_state_dict(W.vae_shapes(decoder=False), 3)
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
    for name, pol, build in cases(E, TorchRefBackend, unet_sd, enc_sd):
        if a.case and not any(c in name for c in a.case):
            continue
        saved = {k: getattr(E, k) for k in pol}
        try:
            for k, v in pol.items():
                setattr(E, k, v)
            plans = build()
        finally:
            for k, v in saved.items():
                setattr(E, k, v)
        for i, plan in enumerate(plans):
            lines = listing(plan)
            tag = name if len(plans) == 1 else f"{name}[{i}]"
            if a.dump:
                with open(os.path.join(a.dump, tag + ".txt"), "w") as f:
                    f.write("\n".join(lines) + "\n")
            print(f"{tag:52s} {len(lines):4d} ops  {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}", flush=True)
        del plans


if __name__ == "__main__":
    main()
