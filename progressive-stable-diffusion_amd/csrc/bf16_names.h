// Included first by every *_bf16.hip twin: selects the bf16 storage type (dadd_common.h) and gives the twin's kernels,
// internal host functions and C entry points their own names, so that the fp16 source compiles a second time beside
// itself in one library.  The fp16 build never sees this header.
#pragma once
#define DADD_BF16 1

#define IgemmArgs IgemmArgs_bf16
#define IgemmLaunch IgemmLaunch_bf16

// kernels (rocprofv3 and the launch tags show the _bf16 names)
#define igemm_kernel igemm_kernel_bf16
#define splitk_finish_kernel splitk_finish_kernel_bf16
#define splitk_finish_gn_kernel splitk_finish_gn_kernel_bf16
#define splitk_finish_gnapply_kernel splitk_finish_gnapply_kernel_bf16
#define igemm_dma_kernel igemm_dma_kernel_bf16
#define igemm_ups_fold_kernel igemm_ups_fold_kernel_bf16
#define conv3x3_halo_kernel conv3x3_halo_kernel_bf16
#define gn_stats_kernel gn_stats_kernel_bf16
#define gn_apply_kernel gn_apply_kernel_bf16
#define gn_fused_kernel gn_fused_kernel_bf16
#define gn_reduce_kernel gn_reduce_kernel_bf16
#define layernorm_kernel layernorm_kernel_bf16
#define flash_kernel flash_kernel_bf16
#define xattn_kernel xattn_kernel_bf16
#define conv_in_nchw_kernel conv_in_nchw_kernel_bf16
#define conv_in_nchw_gn_kernel conv_in_nchw_gn_kernel_bf16
#define conv_cout4_kernel conv_cout4_kernel_bf16
#define wgrad_kernel wgrad_kernel_bf16
#define wgrad_finish_kernel wgrad_finish_kernel_bf16
#define gn_grad_stats_kernel gn_grad_stats_kernel_bf16
#define gn_grad_partial_kernel gn_grad_partial_kernel_bf16
#define gn_grad_apply_kernel gn_grad_apply_kernel_bf16
#define layernorm_grad_kernel layernorm_grad_kernel_bf16
#define geglu_kernel geglu_kernel_bf16
#define geglu_grad_kernel geglu_grad_kernel_bf16
#define attn_grad_stats_kernel attn_grad_stats_kernel_bf16
#define attn_grad_dkv_kernel attn_grad_dkv_kernel_bf16
#define attn_grad_dq_kernel attn_grad_dq_kernel_bf16
#define dgrad_kernel dgrad_kernel_bf16
#define EndWgradArgs EndWgradArgs_bf16
#define end_wgrad_kernel end_wgrad_kernel_bf16
#define end_wgrad_finish_kernel end_wgrad_finish_kernel_bf16
#define gelu_kernel gelu_kernel_bf16
#define gelu_grad_kernel gelu_grad_kernel_bf16
#define gate_tail_kernel gate_tail_kernel_bf16
#define gate_tail_grad_kernel gate_tail_grad_kernel_bf16
#define rowvec_grad_kernel rowvec_grad_kernel_bf16
#define rowvec_grad_finish_kernel rowvec_grad_finish_kernel_bf16
#define relayout_kernel relayout_kernel_bf16
#define plan_refresh_kernel plan_refresh_kernel_bf16

// host functions shared between the GEMM sources and with api.hip
#define dadd_init_igemm dadd_init_igemm_bf16
#define dadd_init_igemm_dma dadd_init_igemm_dma_bf16
#define dadd_igemm_dma_row dadd_igemm_dma_row_bf16
#define dadd_init_igemm_ups_fold dadd_init_igemm_ups_fold_bf16
#define dadd_igemm_ups_fold_row dadd_igemm_ups_fold_row_bf16
#define dadd_igemm_resolve dadd_igemm_resolve_bf16
#define dadd_init_conv_halo dadd_init_conv_halo_bf16
#define dadd_conv_halo_applicable dadd_conv_halo_applicable_bf16
#define dadd_conv_halo_gn_channels dadd_conv_halo_gn_channels_bf16
#define dadd_conv_halo_row dadd_conv_halo_row_bf16
#define dadd_init_norm dadd_init_norm_bf16
#define dadd_init_attention dadd_init_attention_bf16
#define dadd_init_attn_grad dadd_init_attn_grad_bf16

// C entry points (include/dadd_hip.h)
#define dadd_conv_igemm_f16 dadd_conv_igemm_bf16
#define dadd_conv_igemm_resolve_f16 dadd_conv_igemm_resolve_bf16
#define dadd_groupnorm_f16 dadd_groupnorm_bf16
#define dadd_layernorm_f16 dadd_layernorm_bf16
#define dadd_attn_f16 dadd_attn_bf16
#define dadd_attn_debug dadd_attn_debug_bf16      // (diagnostics build only)
#define dadd_self_attn_f16 dadd_self_attn_bf16
#define dadd_tri_xattn_f16 dadd_tri_xattn_bf16
#define dadd_conv_in_nchw_f16 dadd_conv_in_nchw_bf16
#define dadd_conv3x3_cout4_f16 dadd_conv3x3_cout4_bf16
#define dadd_conv_out_ddim_f16 dadd_conv_out_ddim_bf16
#define dadd_conv_wgrad_f16 dadd_conv_wgrad_bf16

// C entry points (include/dadd_hip_norm_grad.h)
#define dadd_groupnorm_grad_f16 dadd_groupnorm_grad_bf16
#define dadd_layernorm_grad_f16 dadd_layernorm_grad_bf16
#define dadd_geglu_f16 dadd_geglu_bf16
#define dadd_geglu_grad_f16 dadd_geglu_grad_bf16

// C entry points (include/dadd_hip_attn_grad.h)
#define dadd_attn_grad_f16 dadd_attn_grad_bf16

// C entry points (include/dadd_hip_cond_grad.h)
#define dadd_gelu_f16 dadd_gelu_bf16
#define dadd_gelu_grad_f16 dadd_gelu_grad_bf16
#define dadd_purifier_gate_tail_f16 dadd_purifier_gate_tail_bf16
#define dadd_purifier_gate_tail_grad_f16 dadd_purifier_gate_tail_grad_bf16

// C entry points (include/dadd_hip_rows_grad.h)
#define dadd_rowvec_grad_f16 dadd_rowvec_grad_bf16

// C entry points (include/dadd_hip_dgrad.h)
#define dadd_conv_dgrad_f16 dadd_conv_dgrad_bf16

// C entry points (include/dadd_hip_end_grad.h)
#define dadd_conv_end_wgrad_f16 dadd_conv_end_wgrad_bf16

// C entry points (include/dadd_hip_relayout.h)
#define dadd_dgrad_relayout_f16 dadd_dgrad_relayout_bf16

// C entry points (include/dadd_hip_plan_refresh.h)
#define dadd_plan_refresh_f16 dadd_plan_refresh_bf16
