/*
 * dadd_hip_metrics.h - the part of libdadd_hip.so's C ABI that carries the evaluation metrics: the CLIP image
 * preprocessing on the device, and the pairwise part of CMMD (unbiased RBF-kernel MMD) and of improved precision /
 * recall (k-th-neighbour manifolds) without an N x N matrix in memory (csrc/metrics.hip; fp32 only, one source).
 * Conventions and status codes are those of dadd_hip.h: plain pointers, sizes and `stream`; every call returns DADD_OK
 * or DADD_EINVAL (contract, see dadd_last_error(); nothing has been launched then) or DADD_EHIP.  No entry point
 * synchronises with the host, and the kernels use no atomics: every sum runs in a fixed order and a call repeated on the
 * same operands gives the same bits.
 *
 * The pair kernels work on PREPARED sets: dadd_feat_prepare_f32 writes copies of the feature rows, centred on one common
 * vector and zero-padded to DADD_METRICS_KPAD columns, and the squared norms of those rows.  A 64 x 64 tile of the Gram
 * matrix g of two prepared sets comes from the fp32-input MFMA (v_mfma_f32_16x16x4_f32: exact fp32 products, one
 * rounding per accumulation, at the fp32 vector rate) with both operands staged through LDS, and
 *   d2(i, j) = max(0, sq_i + sq_j - 2 g(i, j)).
 * Centring leaves every distance as it is and removes the component all rows share, which is what the three terms of d2
 * would otherwise cancel.
 */
#ifndef DADD_HIP_METRICS_H
#define DADD_HIP_METRICS_H

#include "dadd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DADD_METRICS_KPAD 32        /* prepared rows are zero-filled up to the next multiple of this many columns */
#define DADD_METRICS_MAX_SIGMAS 8   /* bandwidths of one dadd_rbf_mmd_f32 call */
#define DADD_METRICS_MAX_K 7        /* neighbourhood size of dadd_knn_radius_f32 */
#define DADD_CLIP_MAX_TAPS 32       /* taps of one coefficient row of dadd_clip_preprocess_u8 */

/* What transformers' CLIPImageProcessor does to an 8-bit image, on the device: u8 NHWC frames in [B][H][W][3] (the layout
 * dadd_frames_to_u8 writes) -> fp32 NCHW out [B][3][S][S].
 *   1. Resize of the shortest edge to S (the other edge to (int)(S * long / short)) with Pillow's antialiased bicubic
 *      filter (a = -0.5): per output pixel and axis, scale = in / out, support = 2 * max(scale, 1), centre =
 *      (o + 0.5) * scale, taps [ (int)(centre - support + 0.5), (int)(centre + support + 0.5) ) clipped to the image,
 *      weight = cubic((tap - centre + 0.5) / max(scale, 1)), normalised to sum 1 per output pixel.
 *   2. Centre crop to S x S (offset (size - S) / 2, rounded down).
 *   3. v / 255, then (v - mean[c]) / std[c]; mean and std are HOST arrays of three.
 * The two passes are separable and run in one kernel: a workgroup owns 16 x 16 output pixels, computes its 2 x 16
 * coefficient rows itself (in double, in the operation order above, so the tap ranges are Pillow's), runs the horizontal
 * pass from global memory into LDS in fp32 and the vertical pass from there.  Nothing is rounded to 8 bits in between.
 * Coefficients are computed on the device rather than tabulated by the host per (H, W, S): 32 lanes of a workgroup spend
 * a few hundred cycles on them, while a host table would need a cache keyed by shape, an upload ordered against the
 * stream, and could not be recorded into a graph.
 * Contract: B, H, W, S >= 1; both scales at most 7 (a coefficient row has at most DADD_CLIP_MAX_TAPS taps); std != 0. */
int dadd_clip_preprocess_u8(const unsigned char* in, float* out, int B, int H, int W, int S, const float* mean,
                            const float* std, void* stream);

/* Scratch every other entry point of this header accepts for sets of n and m rows and S bandwidths (m = 0: one set;
 * S = 0: no dadd_rbf_mmd_f32 call).  Host only.  -1 for sizes the entry points do not take. */
long long dadd_metrics_scratch_bytes(int n, int m, int S);

/* Prepares X [n][D] (leading dimension ldx) and, when y is not null, Y [m][D] (ldy) for the pair kernels.
 *   normalize != 0: every row is first scaled to unit L2 norm (x * (1 / sqrt(sum x^2)), the sum in double).
 *   center [kp], kp = D rounded up to DADD_METRICS_KPAD: the column mean of the (normalised) rows of X, summed in double
 *     in a fixed order (16 interleaved row classes per column, each in row order, then added in class order), zero in
 *     the pad columns.  The SAME vector is subtracted from the rows of Y.
 *   xc [n][ldc], yc [m][ldc]: row - center in columns [0, D), zero in [D, kp); columns from kp on are not touched.
 *   sqx [n], sqy [m]: the squared norm of the fp32 row that was stored, summed in double and rounded once.
 * Contract: n >= 1, m >= 1 when y is given, 1 <= D <= 65536, ldx, ldy >= D, ldc >= kp and a multiple of 4, xc / yc
 * 16-byte aligned, scratch at least dadd_metrics_scratch_bytes(n, m, 0) bytes and 8-byte aligned. */
int dadd_feat_prepare_f32(const float* x, int n, int ldx, const float* y, int m, int ldy, int D, int normalize,
                          float* xc, float* yc, int ldc, float* sqx, float* sqy, float* center, void* scratch,
                          long long scratch_bytes, void* stream);

/* Unbiased MMD^2 with a sum of S RBF kernels exp(-d2 / (2 sigma^2)) between prepared sets xc [n][ldc] and yc [m][ldc].
 * With u = -expm1(-d2 / (2 sigma^2)) = 1 - k, per bandwidth s (sigmas is a HOST array of S):
 *   means[0 * S + s] = sum over i != j of u(x_i, x_j) / (n (n - 1))
 *   means[1 * S + s] = sum over i != j of u(y_i, y_j) / (m (m - 1))
 *   means[2 * S + s] = sum over all i, j of u(x_i, y_j) / (n m)
 *   *mmd2 = - sum over s of (means[0][s] + means[1][s] - 2 means[2][s])
 * which is the estimator on k itself: the ones cancel exactly (1 + 1 - 2), and summing 1 - k keeps the digits that a sum
 * of k ~ 1 loses.  The XX and YY sums visit the upper-triangle tiles only, count the off-diagonal ones twice and mask
 * the diagonal.  Each workgroup writes S double partials to scratch; a finish kernel adds them in workgroup order in
 * double and writes means (3 S doubles) and mmd2 (one double), both on the device.
 * Contract: n, m >= 2 (DADD_EINVAL below: the estimator does not exist), 1 <= S <= DADD_METRICS_MAX_SIGMAS, every sigma
 * > 0, 1 <= D <= ldc, ldc a multiple of 4 and at least D rounded up to DADD_METRICS_KPAD, xc / yc 16-byte aligned,
 * scratch at least dadd_metrics_scratch_bytes(n, m, S) bytes, scratch / means / mmd2 8-byte aligned. */
int dadd_rbf_mmd_f32(const float* xc, const float* sqx, int n, const float* yc, const float* sqy, int m, int D, int ldc,
                     const float* sigmas, int S, double* means, double* mmd2, void* scratch, long long scratch_bytes,
                     void* stream);

/* radius [n]: for every row of the prepared set xc [n][ldc], the (k+1)-th smallest distance (not squared) to the rows of
 * the same set, itself included: torch.cdist(x, x).topk(k + 1, largest=False).values[:, -1].  One workgroup owns 64 rows
 * and walks all column tiles; every lane keeps the 8 smallest (d2, column) pairs of each of its rows in registers, the 16
 * lanes of a row merge theirs through LDS, and the distance to the column that comes out is then recomputed from the
 * differences of the two stored rows in double and rounded once.  Ties in d2 go to the smaller column index.
 * Contract: 1 <= k <= DADD_METRICS_MAX_K, n >= k + 1, D / ldc / alignment as dadd_rbf_mmd_f32. */
int dadd_knn_radius_f32(const float* xc, const float* sqx, int n, int D, int ldc, int k, float* radius, void* stream);

/* hit [nq] (int32): 1 when some row j of the prepared reference set rc [nr][ldc] has d(q_i, r_j) <= radius[j] (compared
 * as d2 <= radius^2 in fp32), else 0.  Both sets must have been centred on the same vector (one dadd_feat_prepare_f32
 * call).  One workgroup owns 64 query rows and walks all reference tiles.
 * Contract: nq, nr >= 1, D / ldc / alignment as dadd_rbf_mmd_f32. */
int dadd_manifold_hits_f32(const float* qc, const float* sqq, int nq, const float* rc, const float* sqr,
                           const float* radius, int nr, int D, int ldc, int* hit, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DADD_HIP_METRICS_H */
