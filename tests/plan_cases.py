"""TEST-ONLY: the plans the CPU checks build on ``TorchRefBackend`` — the case list of scripts/plan_fingerprint.py
(which imports it from here) and of tests/test_igemm_resolve_cpu.py: the benchmark's ``UNetPlan(4, 64)`` and its smaller
siblings in fp16 and bf16, every non-default policy setting the tests and scripts use, and the VAE plans."""
import torch

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


def state_dicts():
    """(UNet + VAE-decoder weights, VAE-encoder weights): seeded, the same for every case."""
    from progressive_stable_diffusion_amd import weights as W
    shapes = dict(W.unet_shapes())
    shapes.update(W.vae_shapes(encoder=False))
    return W.init_state_dict(shapes, 0, gates=GATES), W.init_state_dict(W.vae_shapes(decoder=False), 3)


class policy:
    """Context manager: the engine module ``E`` with the overrides ``pol`` of one case."""

    def __init__(self, E, pol):
        self.E, self.pol = E, pol

    def __enter__(self):
        self.saved = {k: getattr(self.E, k) for k in self.pol}
        for k, v in self.pol.items():
            setattr(self.E, k, v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(self.E, k, v)
