/*
 * dadd_hip_end_grad.h - the part of libdadd_hip.so's C ABI that carries the gradients of the UNet's two 4-channel end
 * convolutions and of the loss (csrc/end_grad.hip, bf16 twin csrc/end_grad_bf16.hip):
 *   conv_in  (fp32 NCHW latents, <= 4 channels -> Cw channels, dadd_conv_in_nchw_*): weight and bias gradient;
 *   conv_out (Cw channels -> <= 4 channels of fp32 NCHW, dadd_conv3x3_cout4_*):      weight and bias gradient;
 *   the row-mean squared error dadd_mse_rows_f32:                                    gradient of pred.
 * The data gradient of conv_out needs no entry point of its own: it is dadd_conv_in_nchw_* run on dy (fp32 NCHW, <= 4
 * channels) with the weight re-laid to [C][9, taps flipped][8]; conv_in's input is data and has no gradient.
 * Conventions and status codes are those of dadd_hip.h: the call launches on `stream` and returns DADD_OK, DADD_EINVAL
 * (contract, see dadd_last_error(); nothing has been launched then) or DADD_EHIP.
 *
 * The algebra.  `thin` is the 4-channel fp32 NCHW tensor [B][Ct][H][W], `wide` the 16-bit NHWC tensor [B][H][W][Cw],
 * r() the rounding to the 16-bit type of the suffix that the forward kernels apply to `thin` on load; both convs are
 * 3x3, stride 1, padding 1, and pixels outside the map contribute zero.
 *   IN  (conv_in:  thin = latents, wide = dy):  dw[n][ky][kx][c] = sum_{b,y,x} wide[b,y,x,n] * r(thin[b,c,y+ky-1,x+kx-1])
 *                                               dbias[n]         = sum_{b,y,x} wide[b,y,x,n]
 *   OUT (conv_out: thin = d pred, wide = x):    dw[o][ky][kx][c] = sum_{b,y,x} r(thin[b,o,y,x]) * wide[b,y+ky-1,x+kx-1,c]
 *                                               dbias[o]         = sum_{b,y,x} r(thin[b,o,y,x])
 * OUT is IN with the taps flipped and the output transposed: one kernel computes
 *   G[tap][t][n] = sum_p wide[p][n] * r(thin[t][p + off(tap)])
 * on MFMA with the pixel p as the reduction index and stores it as dw[n][tap][t] (IN) or dw[t][8 - tap][n] (OUT).
 * Every product of two 16-bit values is exact in fp32; only the fp32 accumulation over M = B*H*W pixels errs.
 */
#ifndef DADD_HIP_END_GRAD_H
#define DADD_HIP_END_GRAD_H

#include <stdint.h>

#include "dadd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DADD_END_WGRAD_IN  0
#define DADD_END_WGRAD_OUT 1

typedef struct {
  const float* thin;   /* [B][Ct][H][W] fp32, dense */
  const void* wide;    /* [B][H][W][Cw] 16-bit, ld_wide elements between pixels (a column slice of wider rows is legal) */
  float* dw;           /* IN: [Cw][9][8], channels c >= Ct written as 0 (the layout of the packed conv_in weight);
                        * OUT: [Ct][9][Cw] (the layout of the packed conv_out weight).  fp32, overwritten */
  float* dbias;        /* IN: [Cw]; OUT: [Ct].  fp32, overwritten; NULL: not computed */
  float* partial;      /* splitm > 1: fp32 scratch of dadd_end_wgrad_partial_floats() elements */
  int32_t B, H, W, Ct, Cw, ld_wide, mode, splitm;
} dadd_end_wgrad_desc;

/* dw and dbias of one end conv.  The M = B*H*W pixels are split over `splitm` workgroups per tile of 64 wide channels;
 * with splitm > 1 every slice writes an fp32 slab into `partial` and a second kernel launched by the same call adds
 * the slabs in slice order (eight runs of consecutive slices, each added in slice order, then the eight runs in a fixed
 * tree).  No floating-point atomics: a call repeated on the same operands gives the same bits.
 * Contract: Cw % 64 == 0; ld_wide % 8 == 0 and ld_wide >= Cw; thin, wide and dw non-NULL, wide, dw and partial 16-byte
 * aligned; 1 <= Ct <= 4; mode DADD_END_WGRAD_IN or _OUT; every size positive and M < 2^31 - 256;
 * 1 <= splitm <= ceil(M / 32); partial non-NULL when splitm > 1. */
int dadd_conv_end_wgrad_f16(const dadd_end_wgrad_desc* d, void* stream);
int dadd_conv_end_wgrad_bf16(const dadd_end_wgrad_desc* d, void* stream);

/* Host only: fp32 elements of `partial` for (mode, Ct, Cw, splitm); 0 for splitm <= 1, -1 for sizes outside the contract. */
long long dadd_end_wgrad_partial_floats(int mode, int Ct, int Cw, int splitm);

/* Backward of dadd_mse_rows_f32: out[b][i] = rowgrad[b] * (2 / per_sample) * (pred[b][i] - target[b][i]), fp32.
 * `rowgrad` [B] is the upstream gradient of the B row means, read on the device (whatever weights the rows - a
 * Min-SNR weight, the 1 / B of a mean, a loss scale - arrives through it).  Contract: pointers non-NULL, B and
 * per_sample positive.  out may be pred itself (in place); it must not overlap target or rowgrad. */
int dadd_mse_rows_grad_f32(const float* pred, const float* target, const float* rowgrad, float* out, int B,
                           int64_t per_sample, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DADD_HIP_END_GRAD_H */
