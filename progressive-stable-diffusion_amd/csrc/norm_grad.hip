// Backward of GroupNorm(+SiLU), LayerNorm and GEGLU, and the plain forward of GEGLU (include/dadd_hip_norm_grad.h) —
// HBM-bound kernels in the manner of norm.hip: wave64, 16-byte loads/stores, fp32 arithmetic, chunk partials combined
// in a fixed order (in double where norm.hip does so), no atomics: results are bit-reproducible run to run.
#include "dadd_common.h"
#include "gelu_phi.h"
#include "../../include/dadd_hip_norm_grad.h"

namespace {

constexpr int GNG_MAXV = 2;        // 16-byte channel vectors per thread: C <= 8*256*2 = 4096
constexpr int GNG_CHUNK_MAX = 64;  // row chunks per sample: few enough that every block combines them itself

struct GnGradArgs {
  const half_t* x1;
  const half_t* x2;
  const half_t* dy;
  const float* gamma;
  const float* beta;
  half_t* dx1;
  half_t* dx2;
  float* st;   // [B][nchunk][groups][2] sum (x - p), sum (x - p)^2 about the group's pivot p
  float* gp;   // [B][nchunk][groups][2] sum dz*gamma, sum dz*gamma*xhat
  float* cp;   // [B][nchunk][C][2]      sum dz, sum dz*xhat
  int C1, C2, C, HW, groups, cg, nchunk, rows_per_chunk, rows_per_block, TV, RP, silu;
  float eps;
};

// Rows and channels per thread as in norm.hip: thread = (channel vector tv of TV, row slot tr of RP); the row chunks of
// the statistics / partials passes and the row blocks of the apply pass.
struct GnGradGeom {
  int TV, RP, nchunk, rows_per_chunk, rows_per_block, nrb;
};
GnGradGeom gng_geom(int B, int HW, int C) {
  GnGradGeom g;
  const int nvec = C / 8;
  g.TV = nvec < 256 ? nvec : 256;
  g.RP = 256 / g.TV;
  int nchunk = HW / (2 * g.RP > 16 ? 2 * g.RP : 16);
  if ((long)B * nchunk < 256) nchunk = HW / (4 * g.RP);      // small maps: one four-row trip per workgroup
  if (nchunk > GNG_CHUNK_MAX) nchunk = GNG_CHUNK_MAX;
  if (nchunk < 1) nchunk = 1;
  g.rows_per_chunk = (HW + nchunk - 1) / nchunk;
  g.nchunk = (HW + g.rows_per_chunk - 1) / g.rows_per_chunk;
  g.rows_per_block = 8 * g.RP;
  if ((long)B * ((HW + g.rows_per_block - 1) / g.rows_per_block) < 256) g.rows_per_block = 4 * g.RP;
  g.nrb = (HW + g.rows_per_block - 1) / g.rows_per_block;
  return g;
}

__device__ __forceinline__ h8 gng_load(const GnGradArgs& p, size_t pix, int c) {
  return (c < p.C1) ? *reinterpret_cast<const h8*>(p.x1 + pix * p.C1 + c)
                    : *reinterpret_cast<const h8*>(p.x2 + pix * p.C2 + (c - p.C1));
}

// dz = dy * silu'(z), silu'(z) = s (1 + z (1 - s)) with s = sigmoid(z) from the forward's v_exp / v_rcp pair
__device__ __forceinline__ float gng_dz(float dy, float z, int silu) {
  if (!silu) return dy;
  const float s = __builtin_amdgcn_rcpf(1.0f + __expf(-z));
  return dy * s * fmaf(z, 1.0f - s, 1.0f);
}

// The (<= 64) chunk partials [nchunk][groups][2] of one sample, summed in double by 8 lanes per group: lane-strided
// partials, then a 3-step butterfly - the order of gn_apply_kernel<true>.  Every lane of a group gets both sums.
__device__ __forceinline__ void gng_combine(const float* part, int nchunk, int groups, int t, double& a, double& q) {
  const int g = t >> 3, sub = t & 7;
  a = 0.0;
  q = 0.0;
  if (g < groups) {
    for (int k = sub; k < nchunk; k += 8) {
      const float2 v = *reinterpret_cast<const float2*>(part + ((size_t)k * groups + g) * 2);
      a += (double)v.x;
      q += (double)v.y;
    }
  }
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    q += __shfl_xor(q, o, 64);
  }
}

// The statistics are summed ABOUT A PIVOT, the first element of the (sample, group) slab: sum (x - p) and sum (x - p)^2.
// E[(x-p)^2] - E[x-p]^2 cancels numbers of the size of the spread, not of the mean, so rstd keeps its accuracy when a
// group sits far from zero.  dgamma needs that: its bound (M + 16) 2^-24 sum |dz xhat| asks about 1e-6 of rstd, which
// plain sums of x and x^2 lose at |mean| = 32 sigma (the forward's 16-bit outputs do not notice 1e-4 of rstd).
__device__ __forceinline__ float gng_pivot(const GnGradArgs& p, int b, int g) {
  const int c = g * p.cg;
  const size_t pix = (size_t)b * p.HW;
  return (float)((c < p.C1) ? p.x1[pix * p.C1 + c] : p.x2[pix * p.C2 + (c - p.C1)]);
}

// mean and rstd of every group of sample b -> lst[2g], lst[2g + 1] (the caller synchronises)
__device__ __forceinline__ void gng_mean_rstd(const GnGradArgs& p, int b, int t, float* lst) {
  double a, q;
  gng_combine(p.st + (size_t)b * p.nchunk * p.groups * 2, p.nchunk, p.groups, t, a, q);
  const int g = t >> 3;
  if (g < p.groups && (t & 7) == 0) {
    const double n = (double)p.HW * (double)p.cg;
    const double d = a / n;                    // mean - pivot
    double var = q / n - d * d;
    if (var < 0.0) var = 0.0;
    lst[2 * g] = (float)((double)gng_pivot(p, b, g) + d);
    lst[2 * g + 1] = (float)(1.0 / sqrt(var + (double)p.eps));
  }
}

// pass 1: per (sample, row chunk) sums of x - p and (x - p)^2 per group, p the group's pivot (gng_pivot); otherwise the
// sums of gn_stats_kernel.  grid (nchunk, B)
template <int NV>
__global__ __launch_bounds__(256) void gn_grad_stats_kernel(const GnGradArgs p) {
  extern __shared__ float sm[];  // [RP][C] sums, [RP][C] squares
  const int t = threadIdx.x, tv = t % p.TV, tr = t / p.TV;
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int row0 = chunk * p.rows_per_chunk;
  const int row1 = min(p.HW, row0 + p.rows_per_chunk);
  const int nvec = p.C >> 3;
  float s[NV][8], ss[NV][8], pv[NV][8];
#pragma unroll
  for (int u = 0; u < NV; ++u)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s[u][e] = ss[u][e] = 0.f;
      const int v = tv + u * p.TV;
      pv[u][e] = (tr < p.RP && v < nvec) ? gng_pivot(p, b, (v * 8 + e) / p.cg) : 0.f;
    }
  if (tr < p.RP) {
    for (int row = row0 + tr; row < row1; row += 4 * p.RP) {   // four rows in flight per thread
      h8 xv[4][NV];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rr = row + q * p.RP;
        const size_t pix = (size_t)b * p.HW + (rr < row1 ? rr : row);
#pragma unroll
        for (int u = 0; u < NV; ++u) {
          const int v = tv + u * p.TV;
          if (v < nvec) xv[q][u] = gng_load(p, pix, v * 8);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (row + q * p.RP >= row1) continue;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
          if (tv + u * p.TV < nvec) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float f = (float)xv[q][u][e] - pv[u][e];
              s[u][e] += f;
              ss[u][e] += f * f;
            }
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int v = tv + u * p.TV;
      if (v < nvec) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          sm[tr * p.C + v * 8 + e] = s[u][e];
          sm[(p.RP + tr) * p.C + v * 8 + e] = ss[u][e];
        }
      }
    }
  }
  __syncthreads();
  const int g = t >> 3, sub = t & 7;     // 8 lanes per group: lane-strided partials, then a 3-step butterfly
  float a = 0.f, q = 0.f;
  if (g < p.groups) {
    const int n = p.RP * p.cg;
    for (int idx = sub; idx < n; idx += 8) {
      const int r = idx / p.cg, c = g * p.cg + (idx - r * p.cg);
      a += sm[r * p.C + c];
      q += sm[(p.RP + r) * p.C + c];
    }
  }
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    q += __shfl_xor(q, o, 64);
  }
  if (g < p.groups && sub == 0) {
    float* w = p.st + (((size_t)b * p.nchunk + chunk) * p.groups + g) * 2;
    w[0] = a;
    w[1] = q;
  }
}

// pass 2: per (sample, row chunk) the channel sums of dz and dz*xhat (-> dbeta, dgamma) and, weighted with gamma, their
// group sums (-> s1, s2 of the apply pass).  Row slots are added in slot order, the channels of a group as in pass 1.
// grid (nchunk, B)
template <int NV>
__global__ __launch_bounds__(256) void gn_grad_partial_kernel(const GnGradArgs p) {
  extern __shared__ float sm[];  // [RP][C][2] channel sums per row slot, [2*groups] mean, rstd
  float* red = sm;
  float* lst = sm + (size_t)2 * p.RP * p.C;
  const int t = threadIdx.x, tv = t % p.TV, tr = t / p.TV;
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int nvec = p.C >> 3;
  gng_mean_rstd(p, b, t, lst);
  __syncthreads();
  float mean[NV][8], rstd[NV][8], gam[NV][8], bet[NV][8], sdz[NV][8], sdx[NV][8];
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int v = tv + u * p.TV;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = v * 8 + e;
      const bool in = v < nvec;
      const int g = in ? c / p.cg : 0;
      mean[u][e] = lst[2 * g];
      rstd[u][e] = lst[2 * g + 1];
      gam[u][e] = in ? p.gamma[c] : 0.f;
      bet[u][e] = in ? p.beta[c] : 0.f;
      sdz[u][e] = sdx[u][e] = 0.f;
    }
  }
  constexpr int ROWS = 4 / NV;     // rows in flight per thread: four 16-byte loads of x and four of dy
  if (tr < p.RP) {
    const int row0 = chunk * p.rows_per_chunk;
    const int row1 = min(p.HW, row0 + p.rows_per_chunk);
    for (int row = row0 + tr; row < row1; row += ROWS * p.RP) {
      h8 xv[ROWS][NV], dv[ROWS][NV];
#pragma unroll
      for (int q = 0; q < ROWS; ++q) {
        const int rr = row + q * p.RP;
        const size_t pix = (size_t)b * p.HW + (rr < row1 ? rr : row);
#pragma unroll
        for (int u = 0; u < NV; ++u) {
          const int v = tv + u * p.TV;
          if (v < nvec) {
            xv[q][u] = gng_load(p, pix, v * 8);
            dv[q][u] = *reinterpret_cast<const h8*>(p.dy + pix * p.C + v * 8);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < ROWS; ++q) {
        if (row + q * p.RP >= row1) continue;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
          if (tv + u * p.TV < nvec) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float xh = ((float)xv[q][u][e] - mean[u][e]) * rstd[u][e];
              const float dz = gng_dz((float)dv[q][u][e], fmaf(xh, gam[u][e], bet[u][e]), p.silu);
              sdz[u][e] += dz;
              sdx[u][e] = fmaf(dz, xh, sdx[u][e]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int v = tv + u * p.TV;
      if (v < nvec) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float* w = red + ((size_t)tr * p.C + v * 8 + e) * 2;
          w[0] = sdz[u][e];
          w[1] = sdx[u][e];
        }
      }
    }
  }
  __syncthreads();
  for (int c = t; c < p.C; c += 256) {       // channel c is this thread's alone from here to the next barrier
    float a = 0.f, q = 0.f;
    for (int r = 0; r < p.RP; ++r) {
      a += red[((size_t)r * p.C + c) * 2];
      q += red[((size_t)r * p.C + c) * 2 + 1];
    }
    *reinterpret_cast<float2*>(p.cp + (((size_t)b * p.nchunk + chunk) * p.C + c) * 2) = float2{a, q};
    const float gm = p.gamma[c];
    red[2 * c] = a * gm;
    red[2 * c + 1] = q * gm;
  }
  __syncthreads();
  const int g = t >> 3, sub = t & 7;
  float a = 0.f, q = 0.f;
  if (g < p.groups) {
    for (int idx = sub; idx < p.cg; idx += 8) {
      a += red[2 * (g * p.cg + idx)];
      q += red[2 * (g * p.cg + idx) + 1];
    }
  }
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    q += __shfl_xor(q, o, 64);
  }
  if (g < p.groups && sub == 0) {
    float* w = p.gp + (((size_t)b * p.nchunk + chunk) * p.groups + g) * 2;
    w[0] = a;
    w[1] = q;
  }
}

// pass 3: every block combines the chunk partials of its sample itself (statistics, then s1 and s2), as the forward's
// apply pass does, and writes dx = rstd * (dz*gamma - (s1 + xhat*s2)/n) for its rows.  grid (row blocks, B)
template <int NV>
__global__ __launch_bounds__(256) void gn_grad_apply_kernel(const GnGradArgs p) {
  extern __shared__ float sm[];  // [2*groups] mean, rstd; [2*groups] s1/n, s2/n
  float* lst = sm;
  float* lsn = sm + 2 * p.groups;
  const int t = threadIdx.x, tv = t % p.TV, tr = t / p.TV;
  const int b = blockIdx.y;
  const int nvec = p.C >> 3;
  gng_mean_rstd(p, b, t, lst);
  {
    double a, q;
    gng_combine(p.gp + (size_t)b * p.nchunk * p.groups * 2, p.nchunk, p.groups, t, a, q);
    const int g = t >> 3;
    if (g < p.groups && (t & 7) == 0) {
      const double n = (double)p.HW * (double)p.cg;
      lsn[2 * g] = (float)(a / n);
      lsn[2 * g + 1] = (float)(q / n);
    }
  }
  __syncthreads();
  if (tr >= p.RP) return;
  float mean[NV][8], rstd[NV][8], gam[NV][8], bet[NV][8], s1n[NV][8], s2n[NV][8];
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int v = tv + u * p.TV;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = v * 8 + e;
      const bool in = v < nvec;
      const int g = in ? c / p.cg : 0;
      mean[u][e] = lst[2 * g];
      rstd[u][e] = lst[2 * g + 1];
      s1n[u][e] = lsn[2 * g];
      s2n[u][e] = lsn[2 * g + 1];
      gam[u][e] = in ? p.gamma[c] : 0.f;
      bet[u][e] = in ? p.beta[c] : 0.f;
    }
  }
  constexpr int ROWS = 4 / NV;
  const int row0 = blockIdx.x * p.rows_per_block;
  const int row1 = min(p.HW, row0 + p.rows_per_block);
  for (int row = row0 + tr; row < row1; row += ROWS * p.RP) {
    h8 xv[ROWS][NV], dv[ROWS][NV];
#pragma unroll
    for (int q = 0; q < ROWS; ++q) {
      const int rr = row + q * p.RP;
      const size_t pix = (size_t)b * p.HW + (rr < row1 ? rr : row);
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const int v = tv + u * p.TV;
        if (v < nvec) {
          xv[q][u] = gng_load(p, pix, v * 8);
          dv[q][u] = *reinterpret_cast<const h8*>(p.dy + pix * p.C + v * 8);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < ROWS; ++q) {
      const int rr = row + q * p.RP;
      if (rr >= row1) continue;
      const size_t pix = (size_t)b * p.HW + rr;
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const int v = tv + u * p.TV;
        if (v < nvec) {
          h8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float xh = ((float)xv[q][u][e] - mean[u][e]) * rstd[u][e];
            const float dz = gng_dz((float)dv[q][u][e], fmaf(xh, gam[u][e], bet[u][e]), p.silu);
            o[e] = (half_t)(rstd[u][e] * (dz * gam[u][e] - fmaf(xh, s2n[u][e], s1n[u][e])));
          }
          const int c = v * 8;
          if (c < p.C1) *reinterpret_cast<h8*>(p.dx1 + pix * p.C1 + c) = o;
          else *reinterpret_cast<h8*>(p.dx2 + pix * p.C2 + (c - p.C1)) = o;
        }
      }
    }
  }
}

// Column sums of the partials part [nterm][C][2] -> dbeta (element 0) and dgamma (element 1), overwritten.  A block takes
// 32 channels; thread (q, channel) adds the terms q, q + 8, ... in double, the eight slices are then added in slice order.
// fp32 only: compiled once, in the fp16 translation unit, and launched by dadd_norm_grad_finish for both storage types and
// for the purifier's gate tail (cond_grad.hip).
#ifndef DADD_BF16
__global__ __launch_bounds__(256) void norm_grad_finish_kernel(const float* __restrict__ part, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, int nterm, int C) {
  __shared__ double red[8][32][2];
  const int t = threadIdx.x, ch = t & 31, q = t >> 5;
  const int c = blockIdx.x * 32 + ch;
  double a = 0.0, d = 0.0;
  if (c < C) {
    for (int k = q; k < nterm; k += 8) {
      const float2 v = *reinterpret_cast<const float2*>(part + ((size_t)k * C + c) * 2);
      a += (double)v.x;
      d += (double)v.y;
    }
  }
  red[q][ch][0] = a;
  red[q][ch][1] = d;
  __syncthreads();
  if (t < 32 && c < C) {
    a = red[0][ch][0];
    d = red[0][ch][1];
#pragma unroll
    for (int s = 1; s < 8; ++s) {
      a += red[s][ch][0];
      d += red[s][ch][1];
    }
    dbeta[c] = (float)a;
    dgamma[c] = (float)d;
  }
}
#endif

// LayerNorm backward: one wave per row with the row in registers, as layernorm_kernel; the grid is bounded and every wave
// strides over rows, keeping the column sums of dy and dy*xhat of its rows in registers.  The four waves of a block add
// theirs in wave order through LDS; the block writes part[block][C][2].
constexpr int LNG_MAXV = 4;       // C <= 8*64*4 = 2048
template <bool DX>
__global__ __launch_bounds__(256) void layernorm_grad_kernel(const half_t* __restrict__ x, const half_t* __restrict__ dy,
                                                             const float* __restrict__ gamma, half_t* __restrict__ dx,
                                                             float* __restrict__ part, int M, int C, float eps) {
  extern __shared__ float sm[];  // [C][2]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = C >> 3;
  const float invc = 1.0f / (float)C;
  float gm[LNG_MAXV][8], sb[LNG_MAXV][8], sg[LNG_MAXV][8];
#pragma unroll
  for (int u = 0; u < LNG_MAXV; ++u) {
    const int i = lane + 64 * u;
    f4 g0 = {0.f, 0.f, 0.f, 0.f}, g1 = {0.f, 0.f, 0.f, 0.f};
    if (i < nvec) {
      g0 = *reinterpret_cast<const f4*>(gamma + i * 8);
      g1 = *reinterpret_cast<const f4*>(gamma + i * 8 + 4);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      gm[u][e] = g0[e];
      gm[u][e + 4] = g1[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) sb[u][e] = sg[u][e] = 0.f;
  }
  for (int row = blockIdx.x * 4 + wave; row < M; row += gridDim.x * 4) {
    const half_t* xr = x + (size_t)row * C;
    const half_t* dr = dy + (size_t)row * C;
    h8 v[LNG_MAXV], d[LNG_MAXV];
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < LNG_MAXV; ++u) {
      const int i = lane + 64 * u;
      if (i < nvec) {
        v[u] = *reinterpret_cast<const h8*>(xr + i * 8);
        d[u] = *reinterpret_cast<const h8*>(dr + i * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < LNG_MAXV; ++u) {
      if (lane + 64 * u < nvec) {
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += (float)v[u][e];
      }
    }
    const float mean = wave_sum(sum) * invc;
    float sq = 0.f;
#pragma unroll
    for (int u = 0; u < LNG_MAXV; ++u) {
      if (lane + 64 * u < nvec) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float c = (float)v[u][e] - mean;
          sq += c * c;
        }
      }
    }
    const float rstd = rsqrtf(wave_sum(sq) * invc + eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int u = 0; u < LNG_MAXV; ++u) {
      if (lane + 64 * u < nvec) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float xh = ((float)v[u][e] - mean) * rstd;
          const float g = (float)d[u][e];
          const float a = g * gm[u][e];
          s1 += a;
          s2 = fmaf(a, xh, s2);
          sb[u][e] += g;
          sg[u][e] = fmaf(g, xh, sg[u][e]);
        }
      }
    }
    if (DX) {
      const float m1 = wave_sum(s1) * invc, m2 = wave_sum(s2) * invc;
#pragma unroll
      for (int u = 0; u < LNG_MAXV; ++u) {
        const int i = lane + 64 * u;
        if (i < nvec) {
          h8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float xh = ((float)v[u][e] - mean) * rstd;
            o[e] = (half_t)(rstd * ((float)d[u][e] * gm[u][e] - fmaf(xh, m2, m1)));
          }
          *reinterpret_cast<h8*>(dx + (size_t)row * C + i * 8) = o;
        }
      }
    }
  }
  if (part == nullptr) return;     // (uniform: data gradient only)
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int u = 0; u < LNG_MAXV; ++u) {
        const int i = lane + 64 * u;
        if (i < nvec) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float* s = sm + (i * 8 + e) * 2;
            s[0] = w == 0 ? sb[u][e] : s[0] + sb[u][e];
            s[1] = w == 0 ? sg[u][e] : s[1] + sg[u][e];
          }
        }
      }
    }
    __syncthreads();
  }
  float* out = part + (size_t)blockIdx.x * C * 2;
  for (int k = threadIdx.x; k < 2 * C; k += 256) out[k] = sm[k];
}

// GEGLU, one thread per 8 outputs.  gelu and its derivative share the erf of dadd_gelu: dadd_gelu_phi (gelu_phi.h).
__global__ __launch_bounds__(256) void geglu_kernel(const half_t* __restrict__ h, half_t* __restrict__ y, int M, int F) {
  const int fv = F >> 3;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)M * fv) return;
  const size_t m = idx / fv;
  const int f = (int)(idx - m * fv) * 8;
  const h8 a = *reinterpret_cast<const h8*>(h + m * 2 * F + f);
  const h8 g = *reinterpret_cast<const h8*>(h + m * 2 * F + F + f);
  h8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)a[e] * dadd_gelu((float)g[e]));
  *reinterpret_cast<h8*>(y + m * F + f) = o;
}

__global__ __launch_bounds__(256) void geglu_grad_kernel(const half_t* __restrict__ h, const half_t* __restrict__ dy,
                                                         half_t* __restrict__ dh, int M, int F) {
  const int fv = F >> 3;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)M * fv) return;
  const size_t m = idx / fv;
  const int f = (int)(idx - m * fv) * 8;
  const h8 a = *reinterpret_cast<const h8*>(h + m * 2 * F + f);
  const h8 g = *reinterpret_cast<const h8*>(h + m * 2 * F + F + f);
  const h8 d = *reinterpret_cast<const h8*>(dy + m * F + f);
  h8 da, dg;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float gf = (float)g[e], df = (float)d[e];
    float Phi, phi;
    dadd_gelu_phi(gf, Phi, phi);
    da[e] = (half_t)(df * gf * Phi);
    dg[e] = (half_t)(df * (float)a[e] * fmaf(gf, phi, Phi));
  }
  *reinterpret_cast<h8*>(dh + m * 2 * F + f) = da;
  *reinterpret_cast<h8*>(dh + m * 2 * F + F + f) = dg;
}

bool gng_sizes_ok(int B, int HW, int C, int groups) {
  return B > 0 && HW > 0 && C > 0 && C % 8 == 0 && C <= 8 * 256 * GNG_MAXV && groups > 0 && groups <= 32 && C % groups == 0;
}

template <int NV>
int gng_launch(const GnGradArgs& p, const GnGradGeom& g, int B, bool want_dx, float* dgamma, float* dbeta, hipStream_t s) {
  const double act = (double)B * p.HW * p.C * 2.0;
  const size_t sm1 = (size_t)2 * p.RP * p.C * sizeof(float);
  const size_t sm2 = sm1 + (size_t)2 * p.groups * sizeof(float);
  const size_t sm3 = (size_t)4 * p.groups * sizeof(float);
  dadd_launch({DADD_KNAME("gn_grad_stats_kernel"), 0.0, act}, gn_grad_stats_kernel<NV>, dim3(p.nchunk, B), dim3(256),
              (unsigned)sm1, s, p);
  DADD_LAUNCH_CHECK();
  dadd_launch({DADD_KNAME("gn_grad_partial_kernel"), 0.0, act * 2.0}, gn_grad_partial_kernel<NV>, dim3(p.nchunk, B), dim3(256),
              (unsigned)sm2, s, p);
  DADD_LAUNCH_CHECK();
  if (want_dx) {
    dadd_launch({DADD_KNAME("gn_grad_apply_kernel"), 0.0, act * 3.0}, gn_grad_apply_kernel<NV>, dim3(g.nrb, B), dim3(256),
                (unsigned)sm3, s, p);
    DADD_LAUNCH_CHECK();
  }
  return dgamma ? dadd_norm_grad_finish(p.cp, dgamma, dbeta, B * p.nchunk, p.C, s) : DADD_OK;
}

}  // namespace

#ifndef DADD_BF16
// host only, one copy for both storage types (the geometry does not depend on the type)
int dadd_norm_grad_finish(const float* part, float* dgamma, float* dbeta, int nterm, int C, hipStream_t s) {
  dadd_launch({"norm_grad_finish_kernel", 0.0, (double)nterm * C * 8.0}, norm_grad_finish_kernel, dim3((C + 31) / 32),
              dim3(256), 0, s, part, dgamma, dbeta, nterm, C);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}

extern "C" long long dadd_groupnorm_grad_ws_floats(int B, int HW, int C, int groups) {
  if (!gng_sizes_ok(B, HW, C, groups)) return -1;
  const GnGradGeom g = gng_geom(B, HW, C);
  return (long long)B * g.nchunk * (4LL * groups + 2LL * C);
}

extern "C" long long dadd_layernorm_grad_ws_floats(int M, int C) {
  if (M <= 0 || C <= 0 || C % 8 != 0 || C > 8 * 64 * LNG_MAXV) return -1;
  return (long long)dadd_row_wave_blocks(M) * C * 2;
}
#endif

extern "C" int dadd_groupnorm_grad_f16(const dadd_gn_grad_desc* d, void* stream) {
  DADD_REQUIRE(d, "groupnorm_grad: null descriptor");
  const int C = d->C1 + d->C2;
  DADD_REQUIRE(d->x1 && d->dy && d->gamma && d->beta && d->ws, "groupnorm_grad: null pointer");
  DADD_REQUIRE(d->C1 > 0 && d->C1 % 8 == 0 && d->C2 >= 0 && d->C2 % 8 == 0, "groupnorm_grad: C1/C2 must be x8");
  DADD_REQUIRE(d->C2 == 0 || d->x2, "groupnorm_grad: C2>0 needs x2");
  DADD_REQUIRE(d->groups > 0 && d->groups <= 32 && C % d->groups == 0,
               "groupnorm_grad: groups must be <= 32 and divide C");
  DADD_REQUIRE(C <= 8 * 256 * GNG_MAXV, "groupnorm_grad: C=%d too large", C);
  DADD_REQUIRE(d->B > 0 && d->HW > 0, "groupnorm_grad: empty input");
  DADD_REQUIRE((d->dgamma != nullptr) == (d->dbeta != nullptr), "groupnorm_grad: dgamma and dbeta come together");
  DADD_REQUIRE(d->dx1 || d->dgamma, "groupnorm_grad: no output");
  DADD_REQUIRE(d->dx1 ? (d->C2 == 0 || d->dx2) : !d->dx2, "groupnorm_grad: dx2 goes with dx1 and C2>0");
  DADD_REQUIRE(dadd_aligned16(d->x1) && dadd_aligned16(d->dy) && (!d->x2 || dadd_aligned16(d->x2)) &&
                   dadd_aligned16(d->dx1) && dadd_aligned16(d->dx2), "groupnorm_grad: pointers must be 16-byte aligned");
  DADD_REQUIRE((((uintptr_t)d->ws) & 7) == 0, "groupnorm_grad: ws must be 8-byte aligned");
  const GnGradGeom g = gng_geom(d->B, d->HW, C);
  GnGradArgs p;
  p.x1 = static_cast<const half_t*>(d->x1);
  p.x2 = static_cast<const half_t*>(d->x2);
  p.dy = static_cast<const half_t*>(d->dy);
  p.gamma = d->gamma;
  p.beta = d->beta;
  p.dx1 = static_cast<half_t*>(d->dx1);
  p.dx2 = static_cast<half_t*>(d->dx2);
  p.st = d->ws;
  p.gp = p.st + (size_t)d->B * g.nchunk * d->groups * 2;
  p.cp = p.gp + (size_t)d->B * g.nchunk * d->groups * 2;
  p.C1 = d->C1; p.C2 = d->C2; p.C = C; p.HW = d->HW; p.groups = d->groups; p.cg = C / d->groups;
  p.nchunk = g.nchunk; p.rows_per_chunk = g.rows_per_chunk; p.rows_per_block = g.rows_per_block;
  p.TV = g.TV; p.RP = g.RP; p.silu = d->silu; p.eps = d->eps;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return C / 8 <= 256 ? gng_launch<1>(p, g, d->B, d->dx1 != nullptr, d->dgamma, d->dbeta, s)
                      : gng_launch<2>(p, g, d->B, d->dx1 != nullptr, d->dgamma, d->dbeta, s);
}

extern "C" int dadd_layernorm_grad_f16(const void* x, const void* dy, const float* gamma, void* dx, float* dgamma,
                                       float* dbeta, float* ws, int M, int C, float eps, void* stream) {
  DADD_REQUIRE(x && dy && gamma, "layernorm_grad: null pointer");
  DADD_REQUIRE(M > 0 && C > 0 && C % 8 == 0 && C <= 8 * 64 * LNG_MAXV,
               "layernorm_grad: C=%d must be a multiple of 8 and <= %d", C, 8 * 64 * LNG_MAXV);
  DADD_REQUIRE((dgamma != nullptr) == (dbeta != nullptr), "layernorm_grad: dgamma and dbeta come together");
  DADD_REQUIRE(dx || dgamma, "layernorm_grad: no output");
  DADD_REQUIRE(!dgamma || ws, "layernorm_grad: dgamma / dbeta need ws");
  DADD_REQUIRE(dadd_aligned16(x) && dadd_aligned16(dy) && dadd_aligned16(dx) && dadd_aligned16(gamma) &&
                   (((uintptr_t)ws) & 7) == 0, "layernorm_grad: pointers must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nblk = dadd_row_wave_blocks(M);
  float* part = dgamma ? ws : nullptr;
  const double bytes = (double)M * C * (dx ? 6.0 : 4.0);
  const unsigned smem = (unsigned)((size_t)2 * C * sizeof(float));
  if (dx)
    dadd_launch({DADD_KNAME("layernorm_grad_kernel") "<true>", 0.0, bytes}, layernorm_grad_kernel<true>, dim3(nblk), dim3(256),
                smem, s, static_cast<const half_t*>(x), static_cast<const half_t*>(dy), gamma, static_cast<half_t*>(dx),
                part, M, C, eps);
  else
    dadd_launch({DADD_KNAME("layernorm_grad_kernel") "<false>", 0.0, bytes}, layernorm_grad_kernel<false>, dim3(nblk), dim3(256),
                smem, s, static_cast<const half_t*>(x), static_cast<const half_t*>(dy), gamma, static_cast<half_t*>(dx),
                part, M, C, eps);
  DADD_LAUNCH_CHECK();
  return dgamma ? dadd_norm_grad_finish(ws, dgamma, dbeta, nblk, C, s) : DADD_OK;
}

extern "C" int dadd_geglu_f16(const void* h, void* y, int M, int F, void* stream) {
  DADD_REQUIRE(h && y, "geglu: null pointer");
  DADD_REQUIRE(M > 0 && F > 0 && F % 8 == 0, "geglu: F=%d must be a multiple of 8", F);
  DADD_REQUIRE(dadd_aligned16(h) && dadd_aligned16(y), "geglu: pointers must be 16-byte aligned");
  const size_t nthread = (size_t)M * (F / 8);
  DADD_REQUIRE((nthread + 255) / 256 <= 0x7fffffffu, "geglu: too many elements");
  dadd_launch({DADD_KNAME("geglu_kernel"), 0.0, (double)M * F * 6.0}, geglu_kernel, dim3((unsigned)((nthread + 255) / 256)),
              dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const half_t*>(h), static_cast<half_t*>(y), M, F);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}

extern "C" int dadd_geglu_grad_f16(const void* h, const void* dy, void* dh, int M, int F, void* stream) {
  DADD_REQUIRE(h && dy && dh, "geglu_grad: null pointer");
  DADD_REQUIRE(M > 0 && F > 0 && F % 8 == 0, "geglu_grad: F=%d must be a multiple of 8", F);
  DADD_REQUIRE(dadd_aligned16(h) && dadd_aligned16(dy) && dadd_aligned16(dh), "geglu_grad: pointers must be 16-byte aligned");
  const size_t nthread = (size_t)M * (F / 8);
  DADD_REQUIRE((nthread + 255) / 256 <= 0x7fffffffu, "geglu_grad: too many elements");
  dadd_launch({DADD_KNAME("geglu_grad_kernel"), 0.0, (double)M * F * 10.0}, geglu_grad_kernel,
              dim3((unsigned)((nthread + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
              static_cast<const half_t*>(h), static_cast<const half_t*>(dy), static_cast<half_t*>(dh), M, F);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}
