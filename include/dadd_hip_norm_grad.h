/*
 * dadd_hip_norm_grad.h - the part of libdadd_hip.so's C ABI that carries the training backward of the normalisation and
 * gating layers: GroupNorm(+SiLU), LayerNorm and GEGLU (csrc/norm_grad.hip, bf16 twin csrc/norm_grad_bf16.hip), and
 * the plain forward of GEGLU that a training step needs.  Conventions and status codes are those of dadd_hip.h:
 * activations are NHWC / token-major in the 16-bit type of the suffix (_f16 or _bf16, same argument lists), gamma,
 * beta and their gradients are fp32, every call launches on `stream` and returns DADD_OK or DADD_EINVAL (contract, see
 * dadd_last_error(); nothing has been launched then) or DADD_EHIP.  The kernels use no atomics: every sum runs in a
 * fixed order and a call repeated on the same operands gives the same bits.
 */
#ifndef DADD_HIP_NORM_GRAD_H
#define DADD_HIP_NORM_GRAD_H

#include "dadd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One GroupNorm(+SiLU) backward.  Pointers first, then ints, then eps. */
typedef struct dadd_gn_grad_desc {
  const void* x1;      /* [B][HW][C1] input of the forward, first source */
  const void* x2;      /* [B][HW][C2] second source of a skip-concat, or NULL when C2 == 0 */
  const void* dy;      /* [B][HW][C]  gradient of the forward's output, C = C1 + C2 */
  const float* gamma;  /* [C] */
  const float* beta;   /* [C] */
  void* dx1;           /* [B][HW][C1] out, or NULL: no data gradient wanted (then dx2 is NULL too) */
  void* dx2;           /* [B][HW][C2] out; needed exactly when dx1 is given and C2 > 0 */
  float* dgamma;       /* [C] out, overwritten; or NULL together with dbeta */
  float* dbeta;        /* [C] out, overwritten */
  float* ws;           /* scratch, dadd_groupnorm_grad_ws_floats() floats, contents irrelevant on entry */
  int B, HW, C1, C2, groups, silu;
  float eps;
} dadd_gn_grad_desc;

/* Backward of dadd_groupnorm_* (y = [silu](xhat * gamma + beta), xhat = (x - mean_bg) * rstd_bg over the HW * C/groups
 * values of a (sample, group)): dx = rstd * (dz * gamma - (s1 + xhat * s2) / n) with dz = dy [* silu'(z)],
 * s1 = sum dz * gamma, s2 = sum dz * gamma * xhat over the (sample, group); dgamma[c] = sum_{b,hw} dz * xhat,
 * dbeta[c] = sum_{b,hw} dz.  Mean and rstd are recomputed from x (fp32 chunk sums of x - p and (x - p)^2 about the slab's
 * first element p, combined in double, max(var, 0): accurate however far from zero the group sits), the forward saves nothing.  Contract as the forward: C1 > 0, C1 and C2 multiples of 8, groups <= 32 dividing C,
 * C <= 4096, x1 / x2 / dy / dx1 / dx2 16-byte aligned, at least one output.  Replaces torch's native_group_norm_backward
 * (+ silu_backward, + the split of the concat gradient) in a training step. */
int dadd_groupnorm_grad_f16(const dadd_gn_grad_desc* d, void* stream);
int dadd_groupnorm_grad_bf16(const dadd_gn_grad_desc* d, void* stream);

/* Host only: the number of floats of `ws` for a dadd_groupnorm_grad_* call of these sizes (either 16-bit type), or -1
 * when the sizes break the contract above.  Layout: [B][nchunk][groups][2] sums of x - p and (x - p)^2, [B][nchunk][groups][2]
 * sums of dz * gamma and dz * gamma * xhat, [B][nchunk][C][2] sums of dz and dz * xhat; nchunk <= 64 row chunks. */
long long dadd_groupnorm_grad_ws_floats(int B, int HW, int C, int groups);

/* Backward of dadd_layernorm_* over the rows of x [M][C]: with a = dy * gamma and xhat = (x - mean) * rstd of the row
 * (recomputed, exact two-pass variance), dx = rstd * (a - mean(a) - xhat * mean(a * xhat)); dgamma[c] = sum_m dy * xhat,
 * dbeta[c] = sum_m dy, overwritten.  dx may be NULL (parameter gradients only); dgamma and dbeta are NULL together
 * (data gradient only).  ws: dadd_layernorm_grad_ws_floats() floats, [nblk][C][2] per-workgroup column sums.
 * Contract: C a multiple of 8, C <= 2048, M >= 1, x / dy / dx / gamma 16-byte aligned.  Replaces torch's
 * native_layer_norm_backward. */
int dadd_layernorm_grad_f16(const void* x, const void* dy, const float* gamma, void* dx, float* dgamma, float* dbeta,
                            float* ws, int M, int C, float eps, void* stream);
int dadd_layernorm_grad_bf16(const void* x, const void* dy, const float* gamma, void* dx, float* dgamma, float* dbeta,
                             float* ws, int M, int C, float eps, void* stream);

/* Host only: floats of `ws` for dadd_layernorm_grad_* (either type), or -1 when M or C break the contract. */
long long dadd_layernorm_grad_ws_floats(int M, int C);

/* GEGLU as a layer of its own: h [M][2F] with the hidden half in [:, :F] and the gate in [:, F:] (the chunk(2) order of
 * the reference model, NOT the interleaved weight rows of DADD_EPI_GEGLU) -> y [M][F] = hidden * gelu(gate), gelu as in
 * the GEMM epilogue (erf of Abramowitz & Stegun 7.1.26).  The inference path has GEGLU only as an epilogue, which keeps
 * no pre-activation; a training step needs h.  Contract: F a multiple of 8, M >= 1, 16-byte aligned pointers.
 * Replaces chunk + F.gelu + mul. */
int dadd_geglu_f16(const void* h, void* y, int M, int F, void* stream);
int dadd_geglu_bf16(const void* h, void* y, int M, int F, void* stream);

/* Backward of dadd_geglu_*: dh[:, :F] = dy * gelu(gate), dh[:, F:] = dy * hidden * (Phi(gate) + gate * phi(gate)), Phi
 * from the same erf as the forward.  dy [M][F], dh [M][2F].  Same contract.  Replaces the autograd of the three torch
 * ops above. */
int dadd_geglu_grad_f16(const void* h, const void* dy, void* dh, int M, int F, void* stream);
int dadd_geglu_grad_bf16(const void* h, const void* dy, void* dh, int M, int F, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DADD_HIP_NORM_GRAD_H */
