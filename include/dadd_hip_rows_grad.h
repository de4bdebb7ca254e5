/*
 * dadd_hip_rows_grad.h - the part of libdadd_hip.so's C ABI that carries the backward of the fp32 row path
 * (csrc/rows_grad.hip, bf16 twin csrc/rows_grad_bf16.hip): the gradients of dadd_linear_rows_f32 (the AOE projector, the
 * time-embedding MLP and the 22 concatenated time_emb_proj layers), of dadd_aoe_interp_f32 (the AOE class table) and of
 * the per-sample row that DADD_EPI_ROWVEC adds in a conv epilogue.  Conventions and status codes are those of dadd_hip.h
 * and dadd_hip_cond_grad.h: plain pointers, every call launches on `stream` and returns DADD_OK or DADD_EINVAL (contract,
 * see dadd_last_error(); nothing has been launched then) or DADD_EHIP.  The kernels use no atomics: every sum runs in a
 * fixed order and a call repeated on the same operands gives the same bits.
 */
#ifndef DADD_HIP_ROWS_GRAD_H
#define DADD_HIP_ROWS_GRAD_H

#include "dadd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Backward of out = act_in(x) w^T + bias (dadd_linear_rows_f32 with act_out = 0).  x fp32 [M][K], the forward's input
 * (the PRE-activation); w [N][K], fp16 or fp32 by w_f32 as in the forward; dy fp32 [M][N].  With a = act_in(x):
 *   dw[n][k] = sum_m dy[m][n] a[m][k]   fp32 [N][K], overwritten, also for an fp16 w: the gradient of the fp32 master
 *   db[n]    = sum_m dy[m][n]           fp32 [N]
 *   dx[m][k] = act_in'(x[m][k]) sum_n dy[m][n] w[n][k]   fp32 [M][K]
 * act_in 0 none, 1 SiLU (act' = s (1 + x (1 - s)), s = 1 / (1 + exp(-x))), 2 exact GELU (act' = Phi + x phi, Phi = erfc(-x /
 * sqrt 2) / 2 from libm, not the A&S polynomial of the 16-bit GELU).  act_in' is evaluated in double and rounded once: both
 * derivatives have a zero next to which an fp32 evaluation has no relative accuracy, and it is M * K values per call.
 * The sums over m run in ascending m; the sum over n runs per strip of rows of w (wave by wave), the strips are then
 * added in strip order by a second launch that also applies act_in'.
 * dx may be NULL; dw and db may be NULL together, or db alone; at least one output.  ws: dadd_linear_rows_grad_ws_floats()
 * floats, needed with dx: the per-strip partial sums [strips][M][K].
 * A workgroup takes one strip of rows of w and one 512-wide tile of K, 8 rows of x per pass: for M <= 8 w is read once and
 * dw written once; later passes re-read the strip and add to the dw the same thread stored.
 * Contract: K a multiple of 8, K <= 2048, M >= 1, N >= 1, act_in in {0, 1, 2}; x, w, dw, dx and ws 16-byte aligned. */
int dadd_linear_rows_grad_f32(const float* x, const void* w, const float* dy, float* dx, float* dw, float* db, float* ws,
                              int M, int K, int N, int act_in, int w_f32, void* stream);

/* Host only: floats of `ws` for dadd_linear_rows_grad_f32, or -1 when M, K or N break the contract. */
long long dadd_linear_rows_grad_ws_floats(int M, int K, int N);

/* Backward of dadd_aoe_interp_f32: labels fp32 [B], dout fp32 [B][D].  lo, hi and frac of a label as the forward forms
 * them (clamp to [0, classes - 1], floor, hi = min(lo + 1, classes - 1)); per column d, with b ascending,
 *   dtable[c]     = sum_b [c = lo_b] (1 - frac_b) dout[b][d] + [c = hi_b] frac_b dout[b][d]
 *   dbase[d]      = sum_c dtable[c]
 *   ddeltas[j][d] = sum_{c > j} dtable[c]     fp32 [classes - 1][D]
 * both overwritten.  One thread per column.  The labels get no gradient.
 * Contract: B >= 1, D >= 1, 2 <= classes <= 16. */
int dadd_aoe_interp_grad_f32(const float* labels, const float* dout, float* dbase, float* ddeltas, int B, int D,
                             int classes, void* stream);

/* Gradient of the row that DADD_EPI_ROWVEC adds: drow[b][c] = sum_p dy[b][p][c] in fp32 from the 16-bit NHWC
 * dy [B][HW][C], overwritten.  A workgroup sums 64 pixels of up to 512 channels into ws; a second launch adds the
 * workgroups' sums in workgroup order.  ws: dadd_rowvec_grad_ws_floats() floats.
 * Contract: C a multiple of 8, B >= 1, HW >= 1, B <= 65535, HW <= 64 * 65535; dy, drow and ws 16-byte aligned. */
int dadd_rowvec_grad_f16(const void* dy, float* drow, float* ws, int B, int HW, int C, void* stream);
int dadd_rowvec_grad_bf16(const void* dy, float* drow, float* ws, int B, int HW, int C, void* stream);

/* Host only: floats of `ws` for dadd_rowvec_grad_* (either type), or -1 when B, HW or C break the contract. */
long long dadd_rowvec_grad_ws_floats(int B, int HW, int C);

#ifdef __cplusplus
}
#endif
#endif /* DADD_HIP_ROWS_GRAD_H */
