// Evaluation metrics on the device (include/dadd_hip_metrics.h): the CLIP image preprocessing, the preparation of feature
// sets, and the three pair kernels (RBF-kernel MMD sums, k-th-neighbour radii, manifold hits) on one 64 x 64 Gram tile of
// the fp32-input MFMA.  fp32 only: there is no 16-bit twin of this source.
#include <limits.h>
#include <math.h>

#include "../../include/dadd_hip_metrics.h"
#include "dadd_common.h"

namespace {

// ================================================================================================ the pair tile
// A workgroup of four waves computes G = A B^T for 64 rows of A and 64 rows of B (both [rows][ld], prepared: centred and
// zero-padded to MT_KC columns).  Wave w owns rows 16 w .. 16 w + 15 of the tile and all 64 columns: four independent
// 16 x 16 accumulators, which is what v_mfma_f32_16x16x4_f32 (32-cycle issue, 40-cycle dependent latency) needs to issue
// back to back.  Operand lane map: A[row l & 15][k = l >> 4], B[k = l >> 4][col l & 15]; result: col = l & 15,
// row = 4 (l >> 4) + reg.  So element acc[ct][r] of lane l is
//   row i0 + 16 w + 4 (l >> 4) + r,   column j0 + 16 ct + (l & 15).
// LDS rows are MT_KC + 4 floats: 16-byte aligned for the loader's float4 stores, and the 16 rows x 4 k of one operand
// read land in 64 different banks (36 r mod 64 runs through the multiples of 4).
// Rows past the end of a set are loaded from its last row (always in bounds) and masked by the caller's epilogue.
constexpr int MT_TILE = 64;
constexpr int MT_KC = DADD_METRICS_KPAD;
constexpr int MT_LDS = MT_KC + 4;
constexpr int MT_BLOCK = 256;
constexpr int MT_KEEP = DADD_METRICS_MAX_K + 1;   // neighbours a lane keeps per row

__device__ __forceinline__ int mt_min(int a, int b) { return a < b ? a : b; }

__device__ __forceinline__ void pair_gram(const float* __restrict__ A, int na, int i0, const float* __restrict__ B, int nb,
                                          int j0, int ld, int kp, float* As, float* Bs, f4 (&acc)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = tid >> 3, lc = (tid & 7) * 4;      // loader: 64 rows x 8 float4 per operand and chunk, two per thread
  const float* a0 = A + (size_t)mt_min(i0 + lr, na - 1) * ld + lc;
  const float* a1 = A + (size_t)mt_min(i0 + lr + 32, na - 1) * ld + lc;
  const float* b0 = B + (size_t)mt_min(j0 + lr, nb - 1) * ld + lc;
  const float* b1 = B + (size_t)mt_min(j0 + lr + 32, nb - 1) * ld + lc;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  const float* ar = As + (16 * w + (lane & 15)) * MT_LDS + (lane >> 4);
  const float* br = Bs + (lane & 15) * MT_LDS + (lane >> 4);
  for (int k0 = 0; k0 < kp; k0 += MT_KC) {
    const f4 va0 = *reinterpret_cast<const f4*>(a0 + k0), va1 = *reinterpret_cast<const f4*>(a1 + k0);
    const f4 vb0 = *reinterpret_cast<const f4*>(b0 + k0), vb1 = *reinterpret_cast<const f4*>(b1 + k0);
    __syncthreads();                                 // the previous chunk has been read
    *reinterpret_cast<f4*>(As + lr * MT_LDS + lc) = va0;
    *reinterpret_cast<f4*>(As + (lr + 32) * MT_LDS + lc) = va1;
    *reinterpret_cast<f4*>(Bs + lr * MT_LDS + lc) = vb0;
    *reinterpret_cast<f4*>(Bs + (lr + 32) * MT_LDS + lc) = vb1;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < MT_KC; kk += 4) {
      const float a = ar[kk];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, br[16 * ct * MT_LDS + kk], acc[ct], 0, 0, 0);
    }
  }
  __syncthreads();                                   // callers that loop over tiles reuse As / Bs at once
}

__device__ __forceinline__ float pair_d2(float sqi, float sqj, float g) { return fmaxf(0.0f, fmaf(-2.0f, g, sqi + sqj)); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ================================================================================================ RBF-kernel MMD
struct MmdArgs {
  const float* x;
  const float* y;
  const float* sqx;
  const float* sqy;
  double* partial;   // [workgroup][S]
  int n, m, ld, kp, S, tx, ty;
  float gamma[DADD_METRICS_MAX_SIGMAS];   // 1 / (2 sigma^2)
};

// Workgroups [0, tx (tx + 1) / 2): upper-triangle tiles of XX; then ty (ty + 1) / 2 of YY; then tx * ty of XY.
__global__ __launch_bounds__(MT_BLOCK) void rbf_mmd_kernel(MmdArgs a) {
  __shared__ __attribute__((aligned(16))) float As[MT_TILE * MT_LDS];
  __shared__ __attribute__((aligned(16))) float Bs[MT_TILE * MT_LDS];
  __shared__ double red[4][DADD_METRICS_MAX_SIGMAS];
  const int nxx = a.tx * (a.tx + 1) / 2, nyy = a.ty * (a.ty + 1) / 2;
  int t = blockIdx.x, ti, tj;
  const float *A, *B, *sqa, *sqb;
  int na, nb;
  bool sym = true;
  if (t < nxx + nyy) {
    int T = a.tx;
    A = a.x; sqa = a.sqx; na = a.n;
    if (t >= nxx) { t -= nxx; T = a.ty; A = a.y; sqa = a.sqy; na = a.m; }
    B = A; sqb = sqa; nb = na;
    ti = 0;
    while (t >= T - ti) { t -= T - ti; ++ti; }     // row ti of the triangle holds T - ti tiles
    tj = ti + t;
  } else {
    t -= nxx + nyy;
    sym = false;
    A = a.x; sqa = a.sqx; na = a.n;
    B = a.y; sqb = a.sqy; nb = a.m;
    ti = t / a.ty;
    tj = t - ti * a.ty;
  }
  const int i0 = ti * MT_TILE, j0 = tj * MT_TILE;
  f4 acc[4];
  pair_gram(A, na, i0, B, nb, j0, a.ld, a.kp, As, Bs, acc);

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ib = i0 + 16 * w + 4 * (lane >> 4);
  float sqi[4], sum[DADD_METRICS_MAX_SIGMAS];
#pragma unroll
  for (int r = 0; r < 4; ++r) sqi[r] = sqa[mt_min(ib + r, na - 1)];
#pragma unroll
  for (int s = 0; s < DADD_METRICS_MAX_SIGMAS; ++s) sum[s] = 0.0f;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int j = j0 + 16 * ct + (lane & 15);
    const float sqj = sqb[mt_min(j, nb - 1)];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ib + r;
      const bool ok = i < na && j < nb && !(sym && i == j);
      const float d2 = ok ? pair_d2(sqi[r], sqj, acc[ct][r]) : 0.0f;     // u(0) = 0: a masked pair adds nothing
#pragma unroll
      for (int s = 0; s < DADD_METRICS_MAX_SIGMAS; ++s)
        if (s < a.S) sum[s] -= expm1f(-d2 * a.gamma[s]);
    }
  }
  const double weight = (sym && ti != tj) ? 2.0 : 1.0;     // an off-diagonal tile of XX / YY stands for its mirror image too
#pragma unroll
  for (int s = 0; s < DADD_METRICS_MAX_SIGMAS; ++s)
    if (s < a.S) {
      const double v = wave_sum_f64((double)sum[s]);
      if (lane == 0) red[w][s] = v;
    }
  __syncthreads();
  if ((int)threadIdx.x < a.S) {
    const int s = threadIdx.x;
    a.partial[(size_t)blockIdx.x * a.S + s] = weight * ((red[0][s] + red[1][s]) + (red[2][s] + red[3][s]));
  }
}

// One workgroup: the 3 S sums of the partials in workgroup order (each lane its strided share in order, then a fixed
// tree), the means and MMD^2.
__global__ __launch_bounds__(MT_BLOCK) void rbf_mmd_finish_kernel(const double* __restrict__ partial, int S, int nxx, int nyy,
                                                                  int nxy, double cxx, double cyy, double cxy,
                                                                  double* __restrict__ means, double* __restrict__ mmd2) {
  __shared__ double buf[MT_BLOCK];
  __shared__ double mean_s[3 * DADD_METRICS_MAX_SIGMAS];
  const int tid = threadIdx.x;
  for (int o = 0; o < 3 * S; ++o) {
    const int seg = o / S, s = o - seg * S;
    const int b0 = seg == 0 ? 0 : seg == 1 ? nxx : nxx + nyy;
    const int b1 = seg == 0 ? nxx : seg == 1 ? nxx + nyy : nxx + nyy + nxy;
    double v = 0.0;
    for (int b = b0 + tid; b < b1; b += MT_BLOCK) v += partial[(size_t)b * S + s];
    buf[tid] = v;
    __syncthreads();
    for (int h = MT_BLOCK / 2; h > 0; h >>= 1) {
      if (tid < h) buf[tid] += buf[tid + h];
      __syncthreads();
    }
    if (tid == 0) {
      const double mean = buf[0] / (seg == 0 ? cxx : seg == 1 ? cyy : cxy);
      mean_s[o] = mean;
      means[o] = mean;
    }
    __syncthreads();
  }
  if (tid == 0) {
    double total = 0.0;
    for (int s = 0; s < S; ++s) total += (mean_s[s] + mean_s[S + s]) - 2.0 * mean_s[2 * S + s];
    *mmd2 = -total;
  }
}

// ================================================================================================ k-th-neighbour radius
// A (d2, column) pair as one 64-bit key: d2 >= 0, so its bit pattern orders like its value, and equal d2 order by column.
__device__ __forceinline__ unsigned long long knn_key(float d2, int j) {
  return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)j;
}
// Insert into an ascending list of MT_KEEP keys (branch-free: the key bubbles through, the largest falls out).
__device__ __forceinline__ void knn_insert(unsigned long long (&best)[MT_KEEP], unsigned long long v) {
#pragma unroll
  for (int q = 0; q < MT_KEEP; ++q) {
    const unsigned long long lo = best[q] < v ? best[q] : v;
    v = best[q] < v ? v : best[q];
    best[q] = lo;
  }
}

__global__ __launch_bounds__(MT_BLOCK) void knn_radius_kernel(const float* __restrict__ x, const float* __restrict__ sq, int n,
                                                              int ld, int kp, int k, float* __restrict__ radius) {
  __shared__ __attribute__((aligned(16))) float As[MT_TILE * MT_LDS];
  __shared__ __attribute__((aligned(16))) float Bs[MT_TILE * MT_LDS];
  __shared__ unsigned long long cand[16][16][MT_KEEP];     // one round: 16 rows x their 16 lanes x MT_KEEP
  __shared__ int chosen[MT_TILE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
  const int i0 = blockIdx.x * MT_TILE, ib = i0 + 16 * w + 4 * g;
  float sqi[4];
  unsigned long long best[4][MT_KEEP];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    sqi[r] = sq[mt_min(ib + r, n - 1)];
#pragma unroll
    for (int q = 0; q < MT_KEEP; ++q) best[r][q] = ~0ull;
  }
  for (int j0 = 0; j0 < n; j0 += MT_TILE) {
    f4 acc[4];
    pair_gram(x, n, i0, x, n, j0, ld, kp, As, Bs, acc);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int j = j0 + 16 * ct + (lane & 15);
      if (j < n) {
        const float sqj = sq[j];
#pragma unroll
        for (int r = 0; r < 4; ++r) knn_insert(best[r], knn_key(pair_d2(sqi[r], sqj, acc[ct][r]), j));
      }
    }
  }
  // merge the 16 lanes of a row, one register row r per round: 16 tile rows (4 waves x 4 lane groups) at a time
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < MT_KEEP; ++q) cand[4 * w + g][lane & 15][q] = best[r][q];
    __syncthreads();
    if (tid < 16) {
      unsigned long long top[MT_KEEP];
#pragma unroll
      for (int q = 0; q < MT_KEEP; ++q) top[q] = ~0ull;
      for (int c = 0; c < 16; ++c)
        for (int q = 0; q < MT_KEEP; ++q) knn_insert(top, cand[tid][c][q]);
      unsigned long long kth = top[0];
#pragma unroll
      for (int q = 1; q < MT_KEEP; ++q) kth = q == k ? top[q] : kth;
      chosen[16 * (tid >> 2) + 4 * (tid & 3) + r] = (int)(unsigned)(kth & 0xffffffffull);     // tile row 16 w + 4 g + r
    }
  }
  __syncthreads();
  // the distance to the chosen column again, from the differences of the stored rows in double: one rounding in all
  for (int rr = 0; rr < 16; ++rr) {
    const int i = i0 + 16 * w + rr;
    if (i >= n) break;                               // uniform in the wave
    int j = mt_min(chosen[16 * w + rr], n - 1);
    j = j < 0 ? 0 : j;                               // (n >= k + 1 keys were inserted: the k-th is a real column)
    const float* xi = x + (size_t)i * ld;
    const float* xj = x + (size_t)j * ld;
    double s = 0.0;
    for (int c = lane; c < kp; c += 64) {
      const double d = (double)xi[c] - (double)xj[c];
      s = fma(d, d, s);
    }
    s = wave_sum_f64(s);
    if (lane == 0) radius[i] = (float)sqrt(s);
  }
}

// ================================================================================================ manifold hits
__global__ __launch_bounds__(MT_BLOCK) void manifold_hits_kernel(const float* __restrict__ q, const float* __restrict__ sqq, int nq,
                                                                 const float* __restrict__ rset, const float* __restrict__ sqr,
                                                                 const float* __restrict__ radius, int nr, int ld, int kp,
                                                                 int* __restrict__ hit) {
  __shared__ __attribute__((aligned(16))) float As[MT_TILE * MT_LDS];
  __shared__ __attribute__((aligned(16))) float Bs[MT_TILE * MT_LDS];
  __shared__ int row_hit[MT_TILE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
  const int i0 = blockIdx.x * MT_TILE, ib = i0 + 16 * w + 4 * g;
  float sqi[4];
  bool any[4] = {false, false, false, false};
#pragma unroll
  for (int r = 0; r < 4; ++r) sqi[r] = sqq[mt_min(ib + r, nq - 1)];
  if (tid < MT_TILE) row_hit[tid] = 0;
  for (int j0 = 0; j0 < nr; j0 += MT_TILE) {
    f4 acc[4];
    pair_gram(q, nq, i0, rset, nr, j0, ld, kp, As, Bs, acc);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int j = j0 + 16 * ct + (lane & 15);
      if (j < nr) {
        const float sqj = sqr[j], rad = radius[j], r2 = rad * rad;
#pragma unroll
        for (int r = 0; r < 4; ++r) any[r] = any[r] || pair_d2(sqi[r], sqj, acc[ct][r]) <= r2;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (any[r]) row_hit[16 * w + 4 * g + r] = 1;     // every writer stores the same value
  __syncthreads();
  if (tid < MT_TILE && i0 + tid < nq) hit[i0 + tid] = row_hit[tid];
}

// ================================================================================================ feature preparation
constexpr int FP_COLS = 64, FP_CLASSES = 16;        // feat_colmean_kernel: columns per workgroup x interleaved row classes

// inv [rows]: 1 / sqrt(sum x^2) per row, one wave per row
__global__ __launch_bounds__(MT_BLOCK) void feat_rownorm_kernel(const float* __restrict__ x, int n, int ldx, const float* __restrict__ y,
                                                                int m, int ldy, int D, float* __restrict__ inv) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (MT_BLOCK / 64) + (threadIdx.x >> 6);
  if (row >= n + m) return;
  const float* p = row < n ? x + (size_t)row * ldx : y + (size_t)(row - n) * ldy;
  double s = 0.0;
  for (int c = lane; c < D; c += 64) s = fma((double)p[c], (double)p[c], s);
  s = wave_sum_f64(s);
  if (lane == 0) inv[row] = (float)(1.0 / sqrt(s));
}

// center [kp]: column means of X (times inv when given).  Thread (class q, column c) adds rows q, q + 16, ... in order,
// then the 16 classes of a column are added in class order.
__global__ __launch_bounds__(FP_COLS* FP_CLASSES) void feat_colmean_kernel(const float* __restrict__ x, int n, int ldx, int D, int kp,
                                                                          const float* __restrict__ inv, float* __restrict__ center) {
  __shared__ double part[FP_CLASSES][FP_COLS];
  const int cl = threadIdx.x & (FP_COLS - 1), q = threadIdx.x / FP_COLS;
  const int c = blockIdx.x * FP_COLS + cl;
  double s = 0.0;
  if (c < D)
    for (int r = q; r < n; r += FP_CLASSES) {
      const float v = x[(size_t)r * ldx + c];
      s += (double)(inv ? v * inv[r] : v);
    }
  part[q][cl] = s;
  __syncthreads();
  if (q == 0 && c < kp) {
    double t = 0.0;
    for (int k = 0; k < FP_CLASSES; ++k) t += part[k][cl];
    center[c] = c < D ? (float)(t / (double)n) : 0.0f;
  }
}

// one wave per row of X then Y: the centred, padded copy and the squared norm of what was stored
__global__ __launch_bounds__(MT_BLOCK) void feat_centre_kernel(const float* __restrict__ x, int n, int ldx, const float* __restrict__ y,
                                                               int m, int ldy, int D, int kp, const float* __restrict__ inv,
                                                               const float* __restrict__ center, float* __restrict__ xc,
                                                               float* __restrict__ yc, int ldc, float* __restrict__ sqx,
                                                               float* __restrict__ sqy) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (MT_BLOCK / 64) + (threadIdx.x >> 6);
  if (row >= n + m) return;
  const bool isx = row < n;
  const float* p = isx ? x + (size_t)row * ldx : y + (size_t)(row - n) * ldy;
  float* o = isx ? xc + (size_t)row * ldc : yc + (size_t)(row - n) * ldc;
  const float scale = inv ? inv[row] : 1.0f;
  double s = 0.0;
  for (int c = lane; c < kp; c += 64) {
    float v = 0.0f;
    if (c < D) v = (inv ? p[c] * scale : p[c]) - center[c];
    o[c] = v;
    s = fma((double)v, (double)v, s);
  }
  s = wave_sum_f64(s);
  if (lane == 0) (isx ? sqx[row] : sqy[row - n]) = (float)s;
}

// ================================================================================================ CLIP preprocessing
constexpr int CP_T = 16;                            // output pixels per workgroup and axis

struct ClipArgs {
  const unsigned char* in;
  float* out;
  int H, W, S, top, left, out_h, out_w, rows_cap;
  double scale_y, scale_x;
  float mean[3], inv_std[3];
};

__device__ __forceinline__ double clip_cubic(double x) {   // Pillow's bicubic_filter, a = -0.5
  const double a = -0.5;
  x = fabs(x);
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
  return 0.0;
}

// Coefficient row of output pixel `o` of an axis with `in_size` input pixels (Pillow's precompute_coeffs, same operation
// order in double and no contraction into fused multiply-adds, so the truncations give its tap range).
__device__ void clip_coeffs(int o, int in_size, double scale, int* first, int* count, float* wrow) {
#pragma clang fp contract(off)
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fs, ss = 1.0 / fs;
  const double centre = (o + 0.5) * scale;
  int lo = (int)(centre - support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(centre + support + 0.5);
  if (hi > in_size) hi = in_size;
  int cnt = hi - lo;
  if (cnt > DADD_CLIP_MAX_TAPS) cnt = DADD_CLIP_MAX_TAPS;     // never with the scales the entry point accepts
  double ww = 0.0;
  for (int t = 0; t < cnt; ++t) ww += clip_cubic((t + lo - centre + 0.5) * ss);
  for (int t = 0; t < DADD_CLIP_MAX_TAPS; ++t)
    wrow[t] = t < cnt ? (float)(clip_cubic((t + lo - centre + 0.5) * ss) / ww) : 0.0f;
  *first = lo;
  *count = cnt;
}

__global__ __launch_bounds__(CP_T* CP_T) void clip_preprocess_kernel(ClipArgs a) {
  extern __shared__ float mid[];                    // [rows_cap][CP_T][3]: the horizontal pass of this tile's input rows
  __shared__ float wx[CP_T][DADD_CLIP_MAX_TAPS], wy[CP_T][DADD_CLIP_MAX_TAPS];
  __shared__ int fx[CP_T], cx[CP_T], fy[CP_T], cy[CP_T];
  const int tid = threadIdx.x, tx = tid & (CP_T - 1), ty = tid / CP_T;
  const int ox0 = blockIdx.x * CP_T, oy0 = blockIdx.y * CP_T, b = blockIdx.z;
  if (tid < CP_T)       // resized-image coordinates of this tile's columns / rows; a tile past the edge repeats the last one
    clip_coeffs(mt_min(ox0 + tid, a.S - 1) + a.left, a.W, a.scale_x, &fx[tid], &cx[tid], wx[tid]);
  else if (tid < 2 * CP_T)
    clip_coeffs(mt_min(oy0 + tid - CP_T, a.S - 1) + a.top, a.H, a.scale_y, &fy[tid - CP_T], &cy[tid - CP_T], wy[tid - CP_T]);
  __syncthreads();
  const int y_lo = fy[0];
  const int rows = mt_min(fy[CP_T - 1] + cy[CP_T - 1] - y_lo, a.rows_cap);
  const unsigned char* img = a.in + (size_t)b * a.H * a.W * 3;
  for (int e = tid; e < rows * CP_T; e += CP_T * CP_T) {
    const int rr = e / CP_T, t = e - rr * CP_T;
    const unsigned char* p = img + ((size_t)(y_lo + rr) * a.W + fx[t]) * 3;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int k = 0; k < cx[t]; ++k) {
      const float wk = wx[t][k];
      s0 = fmaf(wk, (float)p[3 * k], s0);
      s1 = fmaf(wk, (float)p[3 * k + 1], s1);
      s2 = fmaf(wk, (float)p[3 * k + 2], s2);
    }
    float* mo = mid + (size_t)e * 3;
    mo[0] = s0; mo[1] = s1; mo[2] = s2;
  }
  __syncthreads();
  const int ox = ox0 + tx, oy = oy0 + ty;
  if (ox >= a.S || oy >= a.S) return;
  float s[3] = {0.0f, 0.0f, 0.0f};
  const int r0 = fy[ty] - y_lo;
  for (int k = 0; k < cy[ty]; ++k) {
    const float wk = wy[ty][k];
    const float* mi = mid + ((size_t)mt_min(r0 + k, rows - 1) * CP_T + tx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = fmaf(wk, mi[c], s[c]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    a.out[(((size_t)b * 3 + c) * a.S + oy) * a.S + ox] = (s[c] * (1.0f / 255.0f) - a.mean[c]) * a.inv_std[c];
}

// ================================================================================================ host side
inline int mt_tiles(int n) { return (n + MT_TILE - 1) / MT_TILE; }
inline int mt_kp(int D) { return (D + MT_KC - 1) / MT_KC * MT_KC; }
inline long long mt_mmd_blocks(int n, int m) {
  const long long tx = mt_tiles(n), ty = mt_tiles(m);
  return tx * (tx + 1) / 2 + ty * (ty + 1) / 2 + tx * ty;
}
inline bool mt_aligned(const void* p, unsigned a) { return (((uintptr_t)p) & (a - 1)) == 0; }

// the contract every pair kernel shares for one prepared set
#define MT_REQUIRE_SET(op, what, ptr, sq, rows, D, ldc)                                                                          \
  do {                                                                                                                           \
    DADD_REQUIRE((ptr) && (sq), op ": null " what);                                                                              \
    DADD_REQUIRE((D) >= 1 && (ldc) % 4 == 0 && (ldc) >= mt_kp(D), op ": D=%d, ldc=%d: ldc must be a multiple of 4 and at least " \
                 "D rounded up to %d", D, ldc, MT_KC);                                                                            \
    DADD_REQUIRE(dadd_aligned16(ptr) && mt_aligned(sq, 4), op ": " what " must be 16-byte aligned");                              \
    DADD_REQUIRE((rows) >= 1, op ": " what " has %d rows", rows);                                                                 \
  } while (0)

}  // namespace

extern "C" long long dadd_metrics_scratch_bytes(int n, int m, int S) {
  if (n < 1 || m < 0 || S < 0 || S > DADD_METRICS_MAX_SIGMAS) return -1;
  long long bytes = ((long long)n + m) * 4;                              // dadd_feat_prepare_f32: 1 / norm per row
  if (S > 0 && m > 0) {
    const long long mmd = mt_mmd_blocks(n, m) * S * 8;                   // dadd_rbf_mmd_f32: S doubles per workgroup
    if (mmd > bytes) bytes = mmd;
  }
  return (bytes + 255) / 256 * 256;
}

extern "C" int dadd_feat_prepare_f32(const float* x, int n, int ldx, const float* y, int m, int ldy, int D, int normalize,
                                     float* xc, float* yc, int ldc, float* sqx, float* sqy, float* center, void* scratch,
                                     long long scratch_bytes, void* stream) {
  DADD_REQUIRE(x && xc && sqx && center, "feat_prepare: null pointer");
  DADD_REQUIRE(n >= 1 && D >= 1 && D <= 65536 && ldx >= D, "feat_prepare: n=%d, D=%d, ldx=%d out of range", n, D, ldx);
  if (y) {
    DADD_REQUIRE(yc && sqy, "feat_prepare: y given without yc / sqy");
    DADD_REQUIRE(m >= 1 && ldy >= D, "feat_prepare: m=%d, ldy=%d out of range", m, ldy);
  } else {
    m = 0;
  }
  const int kp = mt_kp(D);
  DADD_REQUIRE(ldc % 4 == 0 && ldc >= kp, "feat_prepare: ldc=%d must be a multiple of 4 and at least %d", ldc, kp);
  DADD_REQUIRE(dadd_aligned16(xc) && dadd_aligned16(yc), "feat_prepare: xc / yc must be 16-byte aligned");
  DADD_REQUIRE((long long)n + m <= INT_MAX - MT_BLOCK, "feat_prepare: too many rows");
  const long long need = dadd_metrics_scratch_bytes(n, m, 0);
  DADD_REQUIRE(scratch && mt_aligned(scratch, 8) && scratch_bytes >= need, "feat_prepare: scratch of %lld bytes, %lld needed",
               scratch_bytes, need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* inv = normalize ? static_cast<float*>(scratch) : nullptr;
  const int rows = n + m, row_blocks = (rows + MT_BLOCK / 64 - 1) / (MT_BLOCK / 64);
  const double in_bytes = (double)rows * D * 4.0;
  if (normalize) {
    dadd_launch({"feat_rownorm_kernel", 2.0 * rows * D, in_bytes}, feat_rownorm_kernel, dim3(row_blocks), dim3(MT_BLOCK), 0, s, x,
                n, ldx, y, m, ldy, D, inv);
    DADD_LAUNCH_CHECK();
  }
  dadd_launch({"feat_colmean_kernel", (double)n * D, (double)n * D * 4.0}, feat_colmean_kernel, dim3(kp / FP_COLS + (kp % FP_COLS != 0)),
              dim3(FP_COLS * FP_CLASSES), 0, s, x, n, ldx, D, kp, (const float*)inv, center);
  DADD_LAUNCH_CHECK();
  dadd_launch({"feat_centre_kernel", 3.0 * rows * D, in_bytes + (double)rows * kp * 4.0}, feat_centre_kernel, dim3(row_blocks),
              dim3(MT_BLOCK), 0, s, x, n, ldx, y, m, ldy, D, kp, (const float*)inv, (const float*)center, xc, yc, ldc, sqx, sqy);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}

extern "C" int dadd_rbf_mmd_f32(const float* xc, const float* sqx, int n, const float* yc, const float* sqy, int m, int D,
                                int ldc, const float* sigmas, int S, double* means, double* mmd2, void* scratch,
                                long long scratch_bytes, void* stream) {
  MT_REQUIRE_SET("rbf_mmd", "xc / sqx", xc, sqx, n, D, ldc);
  MT_REQUIRE_SET("rbf_mmd", "yc / sqy", yc, sqy, m, D, ldc);
  DADD_REQUIRE(n >= 2 && m >= 2, "rbf_mmd: n=%d, m=%d: the unbiased estimator needs two rows of each set", n, m);
  DADD_REQUIRE(sigmas && S >= 1 && S <= DADD_METRICS_MAX_SIGMAS, "rbf_mmd: S=%d bandwidths (1..%d)", S, DADD_METRICS_MAX_SIGMAS);
  DADD_REQUIRE(means && mmd2 && mt_aligned(means, 8) && mt_aligned(mmd2, 8), "rbf_mmd: means / mmd2 must be 8-byte aligned");
  const long long blocks = mt_mmd_blocks(n, m);
  DADD_REQUIRE(blocks <= INT_MAX, "rbf_mmd: n=%d, m=%d give too many tiles", n, m);
  const long long need = dadd_metrics_scratch_bytes(n, m, S);
  DADD_REQUIRE(scratch && mt_aligned(scratch, 8) && scratch_bytes >= need, "rbf_mmd: scratch of %lld bytes, %lld needed",
               scratch_bytes, need);
  MmdArgs a;
  a.x = xc; a.y = yc; a.sqx = sqx; a.sqy = sqy;
  a.partial = static_cast<double*>(scratch);
  a.n = n; a.m = m; a.ld = ldc; a.kp = mt_kp(D); a.S = S; a.tx = mt_tiles(n); a.ty = mt_tiles(m);
  for (int s = 0; s < DADD_METRICS_MAX_SIGMAS; ++s) {
    if (s < S) DADD_REQUIRE(sigmas[s] > 0.0f, "rbf_mmd: sigma[%d]=%g must be positive", s, (double)sigmas[s]);
    a.gamma[s] = s < S ? (float)(1.0 / (2.0 * (double)sigmas[s] * (double)sigmas[s])) : 0.0f;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const double pairs = 0.5 * n * n + 0.5 * m * m + (double)n * m;
  dadd_launch({"rbf_mmd_kernel", 2.0 * pairs * a.kp, ((double)n + m) * a.kp * 4.0 + (double)blocks * S * 8.0}, rbf_mmd_kernel,
              dim3((unsigned)blocks), dim3(MT_BLOCK), 0, s, a);
  DADD_LAUNCH_CHECK();
  const int nxx = a.tx * (a.tx + 1) / 2, nyy = a.ty * (a.ty + 1) / 2, nxy = a.tx * a.ty;
  dadd_launch({"rbf_mmd_finish_kernel", 0.0, (double)blocks * S * 8.0}, rbf_mmd_finish_kernel, dim3(1), dim3(MT_BLOCK), 0, s,
              (const double*)a.partial, S, nxx, nyy, nxy, (double)n * (n - 1), (double)m * (m - 1), (double)n * m, means, mmd2);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}

extern "C" int dadd_knn_radius_f32(const float* xc, const float* sqx, int n, int D, int ldc, int k, float* radius, void* stream) {
  MT_REQUIRE_SET("knn_radius", "xc / sqx", xc, sqx, n, D, ldc);
  DADD_REQUIRE(radius && mt_aligned(radius, 4), "knn_radius: null or misaligned radius");
  DADD_REQUIRE(k >= 1 && k <= DADD_METRICS_MAX_K, "knn_radius: k=%d (1..%d)", k, DADD_METRICS_MAX_K);
  DADD_REQUIRE(n >= k + 1, "knn_radius: n=%d rows have no %d-th neighbour", n, k);
  const int kp = mt_kp(D);
  dadd_launch({"knn_radius_kernel", 2.0 * n * n * kp, (double)n * kp * 4.0}, knn_radius_kernel, dim3(mt_tiles(n)), dim3(MT_BLOCK), 0,
              static_cast<hipStream_t>(stream), xc, sqx, n, ldc, kp, k, radius);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}

extern "C" int dadd_manifold_hits_f32(const float* qc, const float* sqq, int nq, const float* rc, const float* sqr,
                                      const float* radius, int nr, int D, int ldc, int* hit, void* stream) {
  MT_REQUIRE_SET("manifold_hits", "qc / sqq", qc, sqq, nq, D, ldc);
  MT_REQUIRE_SET("manifold_hits", "rc / sqr", rc, sqr, nr, D, ldc);
  DADD_REQUIRE(radius && hit && mt_aligned(radius, 4) && mt_aligned(hit, 4), "manifold_hits: null or misaligned radius / hit");
  const int kp = mt_kp(D);
  dadd_launch({"manifold_hits_kernel", 2.0 * nq * nr * kp, ((double)nq + nr) * kp * 4.0}, manifold_hits_kernel, dim3(mt_tiles(nq)),
              dim3(MT_BLOCK), 0, static_cast<hipStream_t>(stream), qc, sqq, nq, rc, sqr, radius, nr, ldc, kp, hit);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}

extern "C" int dadd_clip_preprocess_u8(const unsigned char* in, float* out, int B, int H, int W, int S, const float* mean,
                                       const float* std, void* stream) {
  DADD_REQUIRE(in && out && mean && std, "clip_preprocess: null pointer");
  DADD_REQUIRE(B >= 1 && H >= 1 && W >= 1 && S >= 1 && B <= 65535, "clip_preprocess: B=%d, H=%d, W=%d, S=%d out of range", B, H, W, S);
  DADD_REQUIRE(mt_aligned(out, 4), "clip_preprocess: out must be 4-byte aligned");
  ClipArgs a;
  a.in = in; a.out = out; a.H = H; a.W = W; a.S = S;
  // transformers' get_resize_output_image_size for {"shortest_edge": S}: the short edge S, the long one truncated
  if (H <= W) { a.out_h = S; a.out_w = (int)((double)S * W / H); }
  else        { a.out_w = S; a.out_h = (int)((double)S * H / W); }
  a.top = (a.out_h - S) / 2;
  a.left = (a.out_w - S) / 2;
  a.scale_y = (double)H / a.out_h;
  a.scale_x = (double)W / a.out_w;
  DADD_REQUIRE(a.scale_y <= 7.0 && a.scale_x <= 7.0, "clip_preprocess: %d x %d -> %d shrinks by more than 7", H, W, S);
  for (int c = 0; c < 3; ++c) {
    DADD_REQUIRE(std[c] != 0.0f, "clip_preprocess: std[%d] is zero", c);
    a.mean[c] = mean[c];
    a.inv_std[c] = 1.0f / std[c];
  }
  // input rows under 16 output rows: 15 steps of scale_y between the first and the last centre, a support at each end
  const double fs = a.scale_y < 1.0 ? 1.0 : a.scale_y;
  a.rows_cap = (int)(CP_T * a.scale_y + 4.0 * fs) + 4;
  if (a.rows_cap > H) a.rows_cap = H;
  const unsigned smem = (unsigned)a.rows_cap * CP_T * 3 * sizeof(float);
  const int tiles = (S + CP_T - 1) / CP_T;
  dadd_launch({"clip_preprocess_kernel", 6.0 * B * S * S * 24.0, (double)B * H * W * 3.0 + (double)B * S * S * 12.0},
              clip_preprocess_kernel, dim3(tiles, tiles, B), dim3(CP_T * CP_T), smem, static_cast<hipStream_t>(stream), a);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}
