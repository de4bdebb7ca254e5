/*
 * dadd_hip_cond_grad.h - the part of libdadd_hip.so's C ABI that carries the training kernels of the conditioning
 * front-end (csrc/cond_grad.hip, bf16 twin csrc/cond_grad_bf16.hip): the exact-form GELU as a layer of its own with its
 * derivative, and the FeaturePurifier's tail LayerNorm(img - sigmoid(z) * dis) with its backward.  Conventions and
 * status codes are those of dadd_hip.h and dadd_hip_norm_grad.h: activations are token-major rows in the 16-bit type of
 * the suffix (_f16 or _bf16, same argument lists), gamma, beta and their gradients are fp32, every call launches on
 * `stream` and returns DADD_OK or DADD_EINVAL (contract, see dadd_last_error(); nothing has been launched then) or
 * DADD_EHIP.  The kernels use no atomics: every sum runs in a fixed order and a call repeated on the same operands
 * gives the same bits.
 */
#ifndef DADD_HIP_COND_GRAD_H
#define DADD_HIP_COND_GRAD_H

#include "dadd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* y = gelu(x) over x [M][F], the exact form 0.5 x (1 + erf(x / sqrt 2)) with the erf of Abramowitz & Stegun 7.1.26, in
 * fp32, rounded once: the value DADD_EPI_GELU stores for the same rounded input.  The inference path has this GELU only
 * as a GEMM epilogue, which keeps no pre-activation; a training step needs x.  Contract: F a multiple of 8, M >= 1,
 * 16-byte aligned pointers. */
int dadd_gelu_f16(const void* x, void* y, int M, int F, void* stream);
int dadd_gelu_bf16(const void* x, void* y, int M, int F, void* stream);

/* Backward of dadd_gelu_*: dx = dy * (Phi(x) + x * phi(x)), Phi from the same erf as the forward and phi from the
 * exponential inside it (the helper dadd_geglu_grad_* uses).  x, dy, dx [M][F].  Same contract. */
int dadd_gelu_grad_f16(const void* x, const void* dy, void* dx, int M, int F, void* stream);
int dadd_gelu_grad_bf16(const void* x, const void* dy, void* dx, int M, int F, void* stream);

/* The FeaturePurifier's tail for training: out = LayerNorm(img - sigmoid(z) * dis) * gamma + beta over the rows of
 * [M][C].  img, dis and z are 16-bit, z the gate's PRE-activation (dadd_purifier_tail_f16 takes the gate itself);
 * sigmoid, the statistics (about the row's first element, exact two-pass variance) and the affine run in fp32 and out
 * is fp32 rows.  One wave per row.  Contract: C a multiple of 8, C <= 2048, M >= 1, every pointer 16-byte aligned. */
int dadd_purifier_gate_tail_f16(const void* img, const void* dis, const void* z, const float* gamma, const float* beta,
                                float* out, int M, int C, float eps, void* stream);
int dadd_purifier_gate_tail_bf16(const void* img, const void* dis, const void* z, const float* gamma, const float* beta,
                                 float* out, int M, int C, float eps, void* stream);

/* Backward of dadd_purifier_gate_tail_*, dout fp32 [M][C].  Per row g = sigmoid(z), u = img - g * dis and mean / rstd /
 * xhat of u are recomputed as in the forward; with a = dout * gamma,
 *   du = rstd * (a - mean(a) - xhat * mean(a * xhat)),  dimg = du,  ddis = -g * du,  dz = -du * dis * g * (1 - g),
 *   dgamma[c] = sum_m dout * xhat,  dbeta[c] = sum_m dout (overwritten).
 * Everything is fp32 inside; the 16-bit outputs are rounded once when stored.  Each of dimg / ddis / dz may be NULL;
 * dgamma and dbeta are NULL together; at least one output.  ws: dadd_purifier_gate_tail_grad_ws_floats() floats, needed
 * with dgamma: [nblk][C][2] per-workgroup column sums, added in workgroup order by a second launch.
 * Contract: as the forward; img / dis / z / dout / gamma / dimg / ddis / dz 16-byte aligned, ws 8-byte aligned. */
int dadd_purifier_gate_tail_grad_f16(const void* img, const void* dis, const void* z, const float* dout,
                                     const float* gamma, void* dimg, void* ddis, void* dz, float* dgamma, float* dbeta,
                                     float* ws, int M, int C, float eps, void* stream);
int dadd_purifier_gate_tail_grad_bf16(const void* img, const void* dis, const void* z, const float* dout,
                                      const float* gamma, void* dimg, void* ddis, void* dz, float* dgamma, float* dbeta,
                                      float* ws, int M, int C, float eps, void* stream);

/* Host only: floats of `ws` for dadd_purifier_gate_tail_grad_* (either type), or -1 when M or C break the contract. */
long long dadd_purifier_gate_tail_grad_ws_floats(int M, int C);

#ifdef __cplusplus
}
#endif
#endif /* DADD_HIP_COND_GRAD_H */
