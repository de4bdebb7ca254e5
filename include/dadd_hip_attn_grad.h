/*
 * dadd_hip_attn_grad.h - the part of libdadd_hip.so's C ABI that carries the training backward of attention
 * (csrc/attn_grad.hip, bf16 twin csrc/attn_grad_bf16.hip).  Conventions and status codes are those of dadd_hip.h:
 * token-major tensors in the 16-bit type of the suffix (_f16 or _bf16, same argument list), every call launches on
 * `stream` and returns DADD_OK, DADD_EINVAL (contract, see dadd_last_error(); nothing has been launched then) or
 * DADD_EHIP.  No atomics: every sum runs in a fixed order, a call repeated on the same operands gives the same bits.
 */
#ifndef DADD_HIP_ATTN_GRAD_H
#define DADD_HIP_ATTN_GRAD_H

#include "dadd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One attention backward.  Token (b, n) of a tensor is at ptr + (b * N + n) * ld + head * d, as in dadd_attn_f16; a
 * non-zero bs_* replaces b * N * ld by b * bs (a token range of a longer sequence, e.g. one pathway's 16 tokens of the
 * 48 conditioning tokens).  Pointers first, then the sample strides, then ints, then do_scale. */
typedef struct dadd_attn_grad_desc {
  const void* q;              /* [B][Nq] rows of heads * d columns, row stride ld_q */
  const void* k;              /* [B][Nk], row stride ld_kv */
  const void* v;              /* [B][Nk], row stride ld_kv */
  const void* dout;           /* [B][Nq] gradient of the forward's output, row stride ld_do */
  void* dq;                   /* [B][Nq] out, row stride ld_dq, or NULL: the dq launch is skipped */
  void* dk;                   /* [B][Nk] out, row stride ld_dkv, or NULL */
  void* dv;                   /* [B][Nk] out, row stride ld_dkv, or NULL; dk and dv both NULL: the dkv launch is skipped */
  float* ws;                  /* scratch, dadd_attn_grad_ws_floats() floats, contents irrelevant on entry */
  const float* do_scale_dev;  /* device float or NULL: dout is multiplied by do_scale * (*do_scale_dev) */
  long long bs_q, bs_kv, bs_do, bs_dq, bs_dkv;   /* elements between samples, 0: dense (N * ld) */
  int B, Nq, Nk, heads, d;
  int ld_q, ld_kv, ld_do, ld_dq, ld_dkv;   /* row strides in elements */
  float do_scale;
} dadd_attn_grad_desc;

/* Gradient of O = softmax(Q K^T / sqrt(d)) V per (sample, head) with respect to Q, K and V, given dO = dout * do_scale *
 * (*do_scale_dev) (the scale carries a pathway's gate or lambda without a host read and without a scaled copy of dout).
 * Two-sided flash backward, three launches:
 *   attn_grad_stats : per query row LSE_i (log2 units) and D_i = sum_j P_ij (dO_i . V_j), by the online-softmax
 *                     recurrence over 64-key tiles; neither the forward's output nor a saved LSE is needed;
 *   attn_grad_dkv   : per 64-key tile, over all query tiles: P = exp2(S - LSE), dV += P^T dO, dP = dO V^T,
 *                     dS = P o (dP - D), dK += dS^T Q / sqrt(d);
 *   attn_grad_dq    : per 64-query tile, over all key tiles: dQ += dS K / sqrt(d).
 * Rounding points: S is computed from q * (log2 e / sqrt(d)) rounded to the storage type (as the forward does); P is
 * rounded to the storage type as the operand of P^T dO; dS is computed from the fp32 P, dP and D and rounded to the
 * storage type as the operand of dS^T Q and dS K.  LSE, D, the scale of dout and every accumulator are fp32; each
 * output is rounded once when it is stored.
 * Contract: d in {40, 80, 96, 160}; Nq a multiple of 16, at least 16; Nk any positive count (keys past Nk are masked
 * per key in all three kernels and their rows are neither read nor written; csrc/attn_grad.hip argues every key
 * index); every ld_* a multiple of 8 and at least heads * d; every bs_* a non-negative multiple of 8; all tensor
 * pointers 16-byte aligned; ws non-NULL (8-byte aligned); at least one output.  Outputs must not alias inputs.
 * Columns outside the heads * d of a written row are left untouched. */
int dadd_attn_grad_f16(const dadd_attn_grad_desc* d, void* stream);
int dadd_attn_grad_bf16(const dadd_attn_grad_desc* d, void* stream);

/* Host only: floats of `ws` for these sizes (either 16-bit type), or -1 when a size is not positive.
 * Layout [B][heads][Nq][2]: LSE (log2 units), then D. */
long long dadd_attn_grad_ws_floats(int B, int heads, int Nq);

#ifdef __cplusplus
}
#endif
#endif /* DADD_HIP_ATTN_GRAD_H */
