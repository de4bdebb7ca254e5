"""ctypes binding of ``libdadd_hip.so`` (C ABI declared in ``include/dadd_hip.h``).

There is no fallback: if the library is missing or a symbol is absent, loading raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdadd_hip.so")
CSRC = os.path.join(_HERE, "csrc")
# sources compiled once (fp16 only, or no 16-bit kernel of their own)
_SINGLE_SOURCES = ("attn2_fused", "ffn_block", "tf_head", "conditioning", "api",
                   # training: gradient statistics, clip / loss-scale scalars and the fused AdamW pass (the 16-bit type is a flag)
                   "optim",
                   # evaluation: CLIP preprocessing, feature preparation and the pair kernels of CMMD / precision / recall (fp32 only)
                   "metrics")
# sources compiled a second time as NAME_bf16.hip, the bf16 twin (csrc/bf16_names.h)
_TWINNED_SOURCES = (
    # the UNet's generic-path kernels
    "igemm", "igemm_dma", "conv_halo", "norm", "attention", "elementwise",
    # the upsample convs as four 2x2 phase convs on pre-summed weights (the LDS-DMA ring of igemm_dma_kernel.h, K = 4 Cin)
    "igemm_ups_fold",
    # training backward: the M-reduction GEMM of the weight gradient
    "wgrad",
    # training backward: GroupNorm(+SiLU) / LayerNorm / GEGLU and the plain GEGLU forward
    "norm_grad",
    # training backward: attention (statistics, dK / dV, dQ)
    "attn_grad",
    # training backward: the data gradient of the stride-2 and upsampled 3x3 convs
    "dgrad",
    # training backward: weight / bias gradient of the 4-channel end convs and the loss gradient
    "end_grad",
    # training, conditioning front-end: GELU and its derivative, the purifier's gated tail and its backward
    "cond_grad",
    # training backward of the fp32 row path: linear_rows, aoe_interp and the EPI_ROWVEC row (only the last one is in the twin)
    "rows_grad",
    # training: one-launch re-layout of the 16-bit weights for the data gradients
    "relayout",
    # training -> inference: one-launch refresh of the packed weights of live plans from the fp32 masters
    "plan_refresh")
SOURCES = tuple(s + ".hip" for s in _SINGLE_SOURCES) + tuple(s + sfx for s in _TWINNED_SOURCES for sfx in (".hip", "_bf16.hip"))

DADD_OK, DADD_EINVAL, DADD_EHIP, DADD_ESTATE = 0, -1, -2, -3
EPI_BIAS, EPI_ROWVEC, EPI_RESIDUAL, EPI_GEGLU = 1, 2, 4, 8
EPI_LNFOLD, EPI_QUICKGELU, EPI_GELU, EPI_SIGMOID, EPI_GNSTAT, EPI_LNSTAT = 128, 256, 512, 1024, 2048, 4096
PRE_GN, PRE_GN_SILU = 8192, 16384
EPI_GNAPPLY, EPI_GNAPPLY_SILU = 32768, 65536
TUNE_SHALLOW, TUNE_NODMA, TUNE_PERSIST = 16, 32, 64
TUNE_UPS_FOLD = 131072
XATTN_SPLIT, XATTN_BASELINE = 0, 1
DGRAD_STRIDE2, DGRAD_UPS = 0, 1
END_WGRAD_IN, END_WGRAD_OUT = 0, 1
GN_MAX_CHUNKS = 256

vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


class IgemmDesc(C.Structure):
    """Mirror of ``dadd_igemm_desc``."""
    _fields_ = [(n, vp) for n in ("x", "x2", "w", "out", "partial", "bias", "rowvec", "residual")] + \
               [(n, i32) for n in ("B", "Hi", "Wi", "C1", "C2", "Ho", "Wo", "N", "taps", "stride",
                                   "ups", "pad", "ldo", "ldr", "ld_rowvec", "splitk", "flags",
                                   "tile_n", "tile_m")] + [("counters", vp), ("ln_c1", vp), ("ln_eps", f32), ("gn_ws", vp), ("gn_nchunk", i32), ("gn_cg", i32),
                                                           ("ln_stats_out", vp), ("ln_stats_in", vp), ("ln_parts_out", i32), ("ln_parts_in", i32),
                                                           ("gn_in_ws", vp), ("gn_in_gamma", vp), ("gn_in_beta", vp), ("gn_in_nchunk", i32), ("gn_in_eps", f32),
                                                           ("gn_in_ws2", vp), ("gn_in_nchunk2", i32),
                                                           ("gn_out", vp), ("gn_out_gamma", vp), ("gn_out_beta", vp), ("gn_out_eps", f32),
                                                           ("w_fold", vp)]


class IgemmChoice(C.Structure):
    """Mirror of ``dadd_igemm_choice``: what ``dadd_conv_igemm_*`` would launch for a descriptor."""
    _fields_ = [("kernel", C.c_char_p), ("finish", C.c_char_p)] + \
               [(n, i32) for n in ("tile_m", "tile_n", "nsplit", "kps", "persistent", "grid_x", "grid_y", "block", "smem",
                                   "gm", "gn")]


class WgradDesc(C.Structure):
    """Mirror of ``dadd_wgrad_desc``."""
    _fields_ = [(n, vp) for n in ("dy", "x", "dw", "dbias", "partial")] + \
               [(n, i32) for n in ("B", "Hi", "Wi", "C", "Ho", "Wo", "N", "taps", "stride", "ups", "pad",
                                   "ld_dy", "ld_x", "ld_dw", "ld_tap", "splitm")]


class DgradDesc(C.Structure):
    """Mirror of ``dadd_dgrad_desc``."""
    _fields_ = [(n, vp) for n in ("dy", "wt", "dx")] + \
               [(n, i32) for n in ("B", "Hi", "Wi", "C", "Ho", "Wo", "N", "mode", "ld_dy", "ld_dx")]


class DgradClass(C.Structure):
    """Mirror of ``dadd_dgrad_class``: one parity class of output pixels, its tiles and its run of weight slabs."""
    _fields_ = [(n, i32) for n in ("first_tile", "pixels", "py", "px", "first_slab", "ntaps")]


class DgradChoice(C.Structure):
    """Mirror of ``dadd_dgrad_choice``: what ``dadd_conv_dgrad_*`` would launch for a descriptor."""
    _fields_ = [(n, i32) for n in ("grid_x", "grid_y", "block", "smem", "nclass", "xcd_by_c")] + [("cls", DgradClass * 4)]


class EndWgradDesc(C.Structure):
    """Mirror of ``dadd_end_wgrad_desc``."""
    _fields_ = [(n, vp) for n in ("thin", "wide", "dw", "dbias", "partial")] + \
               [(n, i32) for n in ("B", "H", "W", "Ct", "Cw", "ld_wide", "mode", "splitm")]


class GnGradDesc(C.Structure):
    """Mirror of ``dadd_gn_grad_desc``."""
    _fields_ = [(n, vp) for n in ("x1", "x2", "dy", "gamma", "beta", "dx1", "dx2", "dgamma", "dbeta", "ws")] + \
               [(n, i32) for n in ("B", "HW", "C1", "C2", "groups", "silu")] + [("eps", f32)]


class AttnGradDesc(C.Structure):
    """Mirror of ``dadd_attn_grad_desc``."""
    _fields_ = [(n, vp) for n in ("q", "k", "v", "dout", "dq", "dk", "dv", "ws", "do_scale_dev")] + \
               [(n, i64) for n in ("bs_q", "bs_kv", "bs_do", "bs_dq", "bs_dkv")] + \
               [(n, i32) for n in ("B", "Nq", "Nk", "heads", "d", "ld_q", "ld_kv", "ld_do", "ld_dq", "ld_dkv")] + \
               [("do_scale", f32)]


def _with_bf16(table, stems=None):
    """``table`` with a ``_bf16`` entry behind each ``_f16`` entry of ``stems`` (default: behind every one), carrying the
    prototype of its original: a twin takes the same argument list."""
    out = {}
    for name, proto in table.items():
        out[name] = proto
        if name.endswith("_f16") and (stems is None or name[:-len("_f16")] in stems):
            out[name[:-len("_f16")] + "_bf16"] = proto
    return out


# name -> (restype, argtypes); every symbol include/dadd_hip.h declares
PROTOTYPES = _with_bf16({
    "dadd_last_error": (C.c_char_p, []),
    "dadd_version": (C.c_int, []),
    "dadd_init": (C.c_int, []),
    "dadd_device_info": (C.c_int, [C.c_int, C.POINTER(i64)]),
    "dadd_conv_igemm_f16": (C.c_int, [C.POINTER(IgemmDesc), vp]),
    "dadd_conv_igemm_resolve_f16": (C.c_int, [C.POINTER(IgemmDesc), C.c_int, C.POINTER(IgemmChoice)]),
    "dadd_conv3x3_cin8_f16": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "dadd_conv_in_nchw_f16": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
    "dadd_conv3x3_cout4_f16": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, vp]),
    "dadd_conv_out_ddim_f16": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "dadd_pack_nchw_f32_to_nhwc8_f16": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, f32, vp,
                                                  vp, vp]),
    "dadd_q_sample_f32": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, i64, vp]),
    "dadd_mse_rows_f32": (C.c_int, [vp, vp, vp, C.c_int, i64, vp]),
    "dadd_frames_to_u8": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "dadd_gaussian_sample_f32": (C.c_int, [vp, vp, vp, f32, vp, i64, vp]),
    "dadd_groupnorm_f16": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int,
                                     C.c_int, f32, C.c_int, C.c_int, vp]),
    "dadd_layernorm_f16": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, f32, vp]),
    "dadd_self_attn_f16": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, vp]),
    "dadd_attn2_fused_f16": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, f32, C.c_int, C.c_int, C.c_int, vp]),
    "dadd_ffn_block_f16": (C.c_int, [vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "dadd_ffn_block_bytes": (C.c_int, []),
    "dadd_tf_head_f16": (C.c_int, [vp, vp, vp, C.c_int, vp, vp, f32, vp, vp, vp, f32, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "dadd_tf_head_bytes": (C.c_int, []),
    "dadd_tf_head_debug": (C.c_int, [vp]),
    "dadd_tri_xattn_f16": (C.c_int, [vp, vp, vp, vp, f32, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, vp]),
    "dadd_timestep_features_f32": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    "dadd_linear_rows_f32": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "dadd_attn_f16": (C.c_int, [vp, vp, vp, vp] + [C.c_int] * 8 + [vp]),
    "dadd_clip_patch_rows_f16": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "dadd_aoe_interp_f32": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "dadd_purifier_tail_f16": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, f32, vp]),
    "dadd_conv_wgrad_f16": (C.c_int, [C.POINTER(WgradDesc), vp]),
    "dadd_begin_step": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
    "dadd_ddim_update_f32": (C.c_int, [vp, vp, vp, f32, vp, vp, i64, vp]),
    "dadd_prefetch": (C.c_int, [vp, i64, vp]),
    "dadd_prefetch_join": (C.c_int, [vp]),
    "dadd_graph_begin": (C.c_int, [vp]),
    "dadd_graph_end": (C.c_int, [vp, C.POINTER(vp)]),
    "dadd_graph_launch": (C.c_int, [vp, vp]),
    "dadd_graph_destroy": (C.c_int, [vp]),
    "dadd_prof_begin": (C.c_int, []),
    "dadd_prof_end": (C.c_int, [C.POINTER(C.c_int)]),
    "dadd_prof_record": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double)]),
}, stems=("dadd_conv_igemm", "dadd_conv_in_nchw", "dadd_conv3x3_cout4", "dadd_conv_out_ddim", "dadd_groupnorm", "dadd_layernorm",
          "dadd_self_attn", "dadd_attn", "dadd_tri_xattn"))       # the bf16 siblings this header declares

# every symbol include/dadd_hip_host.h declares (host-only: what a descriptor would launch, csrc/igemm.hip resolve)
HOST_PROTOTYPES = {"dadd_conv_igemm_resolve_bf16": PROTOTYPES["dadd_conv_igemm_resolve_f16"]}

# every symbol include/dadd_hip_grad.h declares (training backward only)
GRAD_PROTOTYPES = {"dadd_conv_wgrad_bf16": PROTOTYPES["dadd_conv_wgrad_f16"]}

# every symbol include/dadd_hip_norm_grad.h declares (training backward of the norms and GEGLU, csrc/norm_grad.hip)
NORM_GRAD_PROTOTYPES = _with_bf16({
    "dadd_groupnorm_grad_f16": (C.c_int, [C.POINTER(GnGradDesc), vp]),
    "dadd_groupnorm_grad_ws_floats": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "dadd_layernorm_grad_f16": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, f32, vp]),
    "dadd_layernorm_grad_ws_floats": (C.c_longlong, [C.c_int, C.c_int]),
    "dadd_geglu_f16": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    "dadd_geglu_grad_f16": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp]),
})

# every symbol include/dadd_hip_attn_grad.h declares (training backward of attention, csrc/attn_grad.hip)
ATTN_GRAD_PROTOTYPES = _with_bf16({
    "dadd_attn_grad_f16": (C.c_int, [C.POINTER(AttnGradDesc), vp]),
    "dadd_attn_grad_ws_floats": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
})

# every symbol include/dadd_hip_dgrad.h declares (data gradient of the stride-2 / upsampled 3x3 conv, csrc/dgrad.hip)
DGRAD_PROTOTYPES = _with_bf16({
    "dadd_conv_dgrad_f16": (C.c_int, [C.POINTER(DgradDesc), vp]),
    "dadd_conv_dgrad_resolve": (C.c_int, [C.POINTER(DgradDesc), C.POINTER(DgradChoice)]),
})

# every symbol include/dadd_hip_end_grad.h declares (gradients of the 4-channel end convs and of the loss, csrc/end_grad.hip)
END_GRAD_PROTOTYPES = _with_bf16({
    "dadd_conv_end_wgrad_f16": (C.c_int, [C.POINTER(EndWgradDesc), vp]),
    "dadd_end_wgrad_partial_floats": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "dadd_mse_rows_grad_f32": (C.c_int, [vp, vp, vp, vp, C.c_int, i64, vp]),
})

# every symbol include/dadd_hip_cond_grad.h declares (training kernels of the conditioning front-end, csrc/cond_grad.hip)
COND_GRAD_PROTOTYPES = _with_bf16({
    "dadd_gelu_f16": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    "dadd_gelu_grad_f16": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp]),
    "dadd_purifier_gate_tail_f16": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, f32, vp]),
    "dadd_purifier_gate_tail_grad_f16": (C.c_int, [vp] * 11 + [C.c_int, C.c_int, f32, vp]),
    "dadd_purifier_gate_tail_grad_ws_floats": (C.c_longlong, [C.c_int, C.c_int]),
})

# every symbol include/dadd_hip_rows_grad.h declares (backward of the fp32 row path, csrc/rows_grad.hip)
ROWS_GRAD_PROTOTYPES = _with_bf16({
    "dadd_linear_rows_grad_f32": (C.c_int, [vp] * 7 + [C.c_int] * 5 + [vp]),
    "dadd_linear_rows_grad_ws_floats": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    "dadd_aoe_interp_grad_f32": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "dadd_rowvec_grad_f16": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "dadd_rowvec_grad_ws_floats": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
})

# include/dadd_hip_optim.h: the optimizer step (csrc/optim.hip)
OPTIM_CHUNK, OPTIM_MAX_GROUPS = 4096, 8
OPTIM_EMA, OPTIM_P16_F16, OPTIM_P16_BF16, OPTIM_ZERO_GRAD = 1, 2, 4, 8


class OptimGroup(C.Structure):
    """Mirror of ``dadd_optim_group``."""
    _fields_ = [(n, f32) for n in ("beta1", "beta2", "eps", "weight_decay", "one_minus_beta1", "one_minus_beta2",
                                   "decay", "step_size", "rsqrt_bc2")] + [("reserved", f32 * 3)]


class OptimState(C.Structure):
    """Mirror of ``dadd_optim_state``, the device-resident block of one optimizer."""
    _fields_ = [(n, i32) for n in ("step", "found_inf", "growth_tracker", "growth_interval", "n_groups")] + \
               [("reserved_i", i32 * 3)] + \
               [(n, f32) for n in ("grad_norm", "coef", "scale", "max_norm", "growth_factor", "backoff_factor")] + \
               [("reserved_f", f32 * 2), ("lr", f32 * OPTIM_MAX_GROUPS), ("group", OptimGroup * OPTIM_MAX_GROUPS)]


# every symbol include/dadd_hip_optim.h declares
OPTIM_PROTOTYPES = {
    "dadd_optim_grad_stats": (C.c_int, [vp, C.c_longlong, vp, vp, C.c_int, vp]),
    "dadd_optim_finalize": (C.c_int, [vp, vp, C.c_longlong, vp, vp]),
    "dadd_optim_adamw_step": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_longlong, C.POINTER(C.c_int), C.c_int, vp, f32,
                                        C.c_int, C.c_int, vp]),
}

# include/dadd_hip_relayout.h: the one-launch re-layout of the data-gradient weights (csrc/relayout.hip)
RELAYOUT_T, RELAYOUT_S2, RELAYOUT_UPS, RELAYOUT_COUT4 = 0, 1, 2, 3
RELAYOUT_TILE = 64


class RelayoutDesc(C.Structure):
    """Mirror of ``dadd_relayout_desc``."""
    _fields_ = [("src_off", C.c_longlong), ("dst_off", C.c_longlong)] + \
               [(n, i32) for n in ("N", "C", "kind", "taps", "tile0", "reserved")]


# every symbol include/dadd_hip_relayout.h declares
RELAYOUT_PROTOTYPES = _with_bf16({
    "dadd_relayout_tiles": (C.c_longlong, [C.c_int] * 4),
    "dadd_relayout_dst_numel": (C.c_longlong, [C.c_int] * 4),
    "dadd_dgrad_relayout_plan": (C.c_longlong, [C.POINTER(RelayoutDesc), C.c_int, C.c_longlong, C.c_longlong]),
    "dadd_dgrad_relayout_f16": (C.c_int, [vp, C.c_longlong, vp, C.c_longlong, vp, C.c_int, C.c_int, vp]),
})

# include/dadd_hip_plan_refresh.h: the one-launch refresh of live plans' packed weights (csrc/plan_refresh.hip)
(PLAN_REFRESH_COPY32, PLAN_REFRESH_CAST, PLAN_REFRESH_GEGLU_W, PLAN_REFRESH_GEGLU_B, PLAN_REFRESH_LNFOLD,
 PLAN_REFRESH_UPSFOLD, PLAN_REFRESH_HEAD_STREAM, PLAN_REFRESH_FFN_STREAM, PLAN_REFRESH_FFN_BIAS) = range(9)
PLAN_REFRESH_GEGLU = 1
PLAN_REFRESH_GROUPS, PLAN_REFRESH_SCALARS, PLAN_REFRESH_ROWS = 1024, 2048, 4


class PlanRefreshDesc(C.Structure):
    """Mirror of ``dadd_plan_refresh_desc``."""
    _fields_ = [("src_off", C.c_longlong * 4), ("dst", vp * 3), ("dst_room", C.c_longlong * 3)] + \
               [(n, i32) for n in ("kind", "N", "K", "Cs", "flags", "wg0")] + [("reserved", i32 * 2)]


# every symbol include/dadd_hip_plan_refresh.h declares
PLAN_REFRESH_PROTOTYPES = _with_bf16({
    "dadd_plan_refresh_wgs": (C.c_longlong, [C.c_int] * 5),
    "dadd_plan_refresh_plan": (C.c_longlong, [C.POINTER(PlanRefreshDesc), C.c_int, C.c_longlong]),
    "dadd_plan_refresh_f16": (C.c_int, [vp, C.c_longlong, vp, C.c_int, C.c_int, vp]),
})

# include/dadd_hip_metrics.h: evaluation metrics (csrc/metrics.hip)
METRICS_KPAD, METRICS_MAX_SIGMAS, METRICS_MAX_K = 32, 8, 7

# every symbol include/dadd_hip_metrics.h declares
METRICS_PROTOTYPES = {
    "dadd_clip_preprocess_u8": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(f32), C.POINTER(f32), vp]),
    "dadd_metrics_scratch_bytes": (C.c_longlong, [C.c_int] * 3),
    "dadd_feat_prepare_f32": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp,
                                        vp, C.c_longlong, vp]),
    "dadd_rbf_mmd_f32": (C.c_int, [vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(f32), C.c_int, vp, vp, vp,
                                   C.c_longlong, vp]),
    "dadd_knn_radius_f32": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "dadd_manifold_hits_f32": (C.c_int, [vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
}

# The registry: header under include/ -> the table of what it declares.  A new header is one entry here; load(), the
# dependencies of build() and the symbol check of __graft_entry__.build() follow.
HEADER_PROTOTYPES = {
    "dadd_hip.h": PROTOTYPES,
    "dadd_hip_host.h": HOST_PROTOTYPES,
    "dadd_hip_grad.h": GRAD_PROTOTYPES,
    "dadd_hip_norm_grad.h": NORM_GRAD_PROTOTYPES,
    "dadd_hip_attn_grad.h": ATTN_GRAD_PROTOTYPES,
    "dadd_hip_dgrad.h": DGRAD_PROTOTYPES,
    "dadd_hip_end_grad.h": END_GRAD_PROTOTYPES,
    "dadd_hip_cond_grad.h": COND_GRAD_PROTOTYPES,
    "dadd_hip_rows_grad.h": ROWS_GRAD_PROTOTYPES,
    "dadd_hip_optim.h": OPTIM_PROTOTYPES,
    "dadd_hip_relayout.h": RELAYOUT_PROTOTYPES,
    "dadd_hip_plan_refresh.h": PLAN_REFRESH_PROTOTYPES,
    "dadd_hip_metrics.h": METRICS_PROTOTYPES,
}
ALL_PROTOTYPES = {}
for _header, _table in HEADER_PROTOTYPES.items():
    assert not ALL_PROTOTYPES.keys() & _table.keys(), (_header, sorted(ALL_PROTOTYPES.keys() & _table.keys()))
    ALL_PROTOTYPES.update(_table)

_lib: Optional[C.CDLL] = None


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 into ``libdadd_hip.so`` (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    import glob
    deps = sorted(set(srcs + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")))) + \
        [os.path.join(os.path.dirname(_HERE), "include", h) for h in HEADER_PROTOTYPES]
    if (not force and os.path.exists(LIB_PATH)
            and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(d) for d in deps)):
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # -amdgpu-mfma-vgpr-form: keep MFMA accumulators in VGPRs.  With the default AGPR form the
    # attention softmax paid 144 v_accvgpr_read/write per 64-key tile (more than half of its VALU).
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-mllvm",
           "-amdgpu-mfma-vgpr-form=1", *os.environ.get("DADD_EXTRA_CFLAGS", "").split(), *srcs, "-o", LIB_PATH]   # (extra flags: diagnostics builds)
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return LIB_PATH


def load() -> C.CDLL:
    """Load the library and bind every prototype; raises RuntimeError when it cannot."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  torch's bundled HIP runtime must be the one in the process: load it first
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension is required (run __graft_entry__.build()); "
            "there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in ALL_PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f"libdadd_hip.so does not export {name}") from e
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc: int) -> None:
    """Map a status code to the exception the reference would raise for the same condition."""
    if rc == DADD_OK:
        return
    msg = (_lib.dadd_last_error() or b"").decode() if _lib is not None else ""
    if rc == DADD_EINVAL:
        raise ValueError(msg)
    raise RuntimeError(f"libdadd_hip error {rc}: {msg}")
