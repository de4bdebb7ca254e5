// Training kernels of the conditioning front-end (include/dadd_hip_cond_grad.h): the exact-form GELU as a layer of its
// own and its derivative (the two MLPs of the Perceiver resampler and of the FeaturePurifier's gate), and the purifier's
// tail LayerNorm(img - sigmoid(z) * dis) with its backward.  HBM-bound kernels in the manner of norm_grad.hip: wave64,
// 16-byte loads / stores, fp32 arithmetic, one wave per row with the row in registers, per-workgroup column sums added
// in workgroup order by a second launch, no atomics: results are bit-reproducible run to run.
#include "dadd_common.h"
#include "gelu_phi.h"
#include "../../include/dadd_hip_cond_grad.h"

namespace {

// ---- GELU, one thread per 8 elements ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gelu_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, size_t nvec) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nvec) return;
  const h8 a = *reinterpret_cast<const h8*>(x + idx * 8);
  h8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (half_t)dadd_gelu((float)a[e]);
  *reinterpret_cast<h8*>(y + idx * 8) = o;
}

__global__ __launch_bounds__(256) void gelu_grad_kernel(const half_t* __restrict__ x, const half_t* __restrict__ dy,
                                                        half_t* __restrict__ dx, size_t nvec) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nvec) return;
  const h8 a = *reinterpret_cast<const h8*>(x + idx * 8);
  const h8 d = *reinterpret_cast<const h8*>(dy + idx * 8);
  h8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float xf = (float)a[e];
    float Phi, phi;
    dadd_gelu_phi(xf, Phi, phi);
    o[e] = (half_t)((float)d[e] * fmaf(xf, phi, Phi));
  }
  *reinterpret_cast<h8*>(dx + idx * 8) = o;
}

// ---- the purifier's tail ----------------------------------------------------------------------------------------------
// One wave per row, the row in registers (C <= 8 * 64 * GT_MAXV).  u = img - g * dis with g = sigmoid(z) in fp32 is formed
// ABOUT A PIVOT, the row's first img element p: c = (img - p) - g * dis (the difference of two 16-bit values of one row
// is exact in fp32, the fma rounds once at the size of the spread), then mean(c), d = c - mean(c), var = mean(d^2) (exact
// two-pass) and xhat = d * rstd.  A row that sits at 50 with a spread of 0.1 keeps xhat to fp32 accuracy of the spread,
// not of the mean: the fp32 output (absolute 2e-5) and dgamma ((M + 16) 2^-24 sum |dout xhat|) both need that.
constexpr int GT_MAXV = 4;       // C <= 2048

__device__ __forceinline__ float gt_sigmoid(float z) { return __builtin_amdgcn_rcpf(1.0f + __expf(-z)); }

// d[u][e] = u - mean(u) of row `row` and rstd; dv / zv keep the row's dis and z for the caller
__device__ __forceinline__ void gt_row(const half_t* __restrict__ img, const half_t* __restrict__ dis,
                                       const half_t* __restrict__ z, size_t row, int C, int lane, float eps,
                                       float (&d)[GT_MAXV][8], h8 (&dv)[GT_MAXV], h8 (&zv)[GT_MAXV], float& rstd) {
  const int nvec = C >> 3;
  const float invc = 1.0f / (float)C;
  const float pivot = (float)img[row * C];
  h8 av[GT_MAXV];
#pragma unroll
  for (int u = 0; u < GT_MAXV; ++u) {
    const int i = lane + 64 * u;
    if (i < nvec) {
      av[u] = *reinterpret_cast<const h8*>(img + row * C + i * 8);
      dv[u] = *reinterpret_cast<const h8*>(dis + row * C + i * 8);
      zv[u] = *reinterpret_cast<const h8*>(z + row * C + i * 8);
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int u = 0; u < GT_MAXV; ++u) {
    if (lane + 64 * u < nvec) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        d[u][e] = fmaf(-gt_sigmoid((float)zv[u][e]), (float)dv[u][e], (float)av[u][e] - pivot);
        sum += d[u][e];
      }
    }
  }
  const float mean = wave_sum(sum) * invc;
  float sq = 0.f;
#pragma unroll
  for (int u = 0; u < GT_MAXV; ++u) {
    if (lane + 64 * u < nvec) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        d[u][e] -= mean;
        sq = fmaf(d[u][e], d[u][e], sq);
      }
    }
  }
  rstd = rsqrtf(wave_sum(sq) * invc + eps);
}

__global__ __launch_bounds__(256) void gate_tail_kernel(const half_t* __restrict__ img, const half_t* __restrict__ dis,
                                                        const half_t* __restrict__ z, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ out, int M,
                                                        int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;      // (a whole wave)
  const int nvec = C >> 3;
  float d[GT_MAXV][8], rstd;
  h8 dv[GT_MAXV], zv[GT_MAXV];
  gt_row(img, dis, z, (size_t)row, C, lane, eps, d, dv, zv, rstd);
#pragma unroll
  for (int u = 0; u < GT_MAXV; ++u) {
    const int i = lane + 64 * u;
    if (i < nvec) {
      float gm[8], bt[8];
      dadd_load8(gamma + i * 8, gm);
      dadd_load8(beta + i * 8, bt);
      f4 o0, o1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o0[e] = fmaf(d[u][e] * rstd, gm[e], bt[e]);
        o1[e] = fmaf(d[u][e + 4] * rstd, gm[e + 4], bt[e + 4]);
      }
      float* o = out + (size_t)row * C + i * 8;
      *reinterpret_cast<f4*>(o) = o0;
      *reinterpret_cast<f4*>(o + 4) = o1;
    }
  }
}

// Backward: the grid is bounded and every wave strides over rows, keeping the column sums of dout and dout * xhat of its
// rows in registers (layernorm_grad_kernel's scheme).  The four waves of a block add theirs in wave order through LDS; the
// block writes part[block][C][2], which dadd_norm_grad_finish (norm_grad.hip) sums into dgamma / dbeta.  dimg / ddis / dz
// may each be NULL; part NULL: no parameter gradients.
__global__ __launch_bounds__(256) void gate_tail_grad_kernel(const half_t* __restrict__ img, const half_t* __restrict__ dis,
                                                             const half_t* __restrict__ z, const float* __restrict__ dout,
                                                             const float* __restrict__ gamma, half_t* __restrict__ dimg,
                                                             half_t* __restrict__ ddis, half_t* __restrict__ dz,
                                                             float* __restrict__ part, int M, int C, float eps) {
  extern __shared__ float sm[];  // [C][2]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = C >> 3;
  const float invc = 1.0f / (float)C;
  const bool want_dx = dimg != nullptr || ddis != nullptr || dz != nullptr;
  float gm[GT_MAXV][8], sb[GT_MAXV][8], sg[GT_MAXV][8];
#pragma unroll
  for (int u = 0; u < GT_MAXV; ++u) {
    const int i = lane + 64 * u;
#pragma unroll
    for (int e = 0; e < 8; ++e) gm[u][e] = sb[u][e] = sg[u][e] = 0.f;
    if (i < nvec) dadd_load8(gamma + i * 8, gm[u]);
  }
  for (int row = blockIdx.x * 4 + wave; row < M; row += gridDim.x * 4) {
    float d[GT_MAXV][8], go[GT_MAXV][8], rstd;
    h8 dv[GT_MAXV], zv[GT_MAXV];
#pragma unroll
    for (int u = 0; u < GT_MAXV; ++u) {
      const int i = lane + 64 * u;
      if (i < nvec) dadd_load8(dout + (size_t)row * C + i * 8, go[u]);
    }
    gt_row(img, dis, z, (size_t)row, C, lane, eps, d, dv, zv, rstd);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int u = 0; u < GT_MAXV; ++u) {
      if (lane + 64 * u < nvec) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float xh = d[u][e] * rstd;
          const float a = go[u][e] * gm[u][e];
          s1 += a;
          s2 = fmaf(a, xh, s2);
          sb[u][e] += go[u][e];
          sg[u][e] = fmaf(go[u][e], xh, sg[u][e]);
        }
      }
    }
    if (want_dx) {     // (uniform)
      const float m1 = wave_sum(s1) * invc, m2 = wave_sum(s2) * invc;
#pragma unroll
      for (int u = 0; u < GT_MAXV; ++u) {
        const int i = lane + 64 * u;
        if (i < nvec) {
          h8 oi, od, oz;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float xh = d[u][e] * rstd;
            const float du = rstd * (go[u][e] * gm[u][e] - fmaf(xh, m2, m1));
            const float g = gt_sigmoid((float)zv[u][e]);
            const float dd = -g * du;
            oi[e] = (half_t)du;
            od[e] = (half_t)dd;
            oz[e] = (half_t)(dd * (float)dv[u][e] * (1.0f - g));
          }
          const size_t off = (size_t)row * C + i * 8;
          if (dimg != nullptr) *reinterpret_cast<h8*>(dimg + off) = oi;
          if (ddis != nullptr) *reinterpret_cast<h8*>(ddis + off) = od;
          if (dz != nullptr) *reinterpret_cast<h8*>(dz + off) = oz;
        }
      }
    }
  }
  if (part == nullptr) return;     // (uniform: data gradients only)
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int u = 0; u < GT_MAXV; ++u) {
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
  float* o = part + (size_t)blockIdx.x * C * 2;
  for (int k = threadIdx.x; k < 2 * C; k += 256) o[k] = sm[k];
}

bool gt_sizes_ok(int M, int C) { return M > 0 && C > 0 && C % 8 == 0 && C <= 8 * 64 * GT_MAXV; }

}  // namespace

#ifndef DADD_BF16
// host only, one copy for both storage types
extern "C" long long dadd_purifier_gate_tail_grad_ws_floats(int M, int C) {
  if (!gt_sizes_ok(M, C)) return -1;
  return (long long)dadd_row_wave_blocks(M) * C * 2;
}
#endif

extern "C" int dadd_gelu_f16(const void* x, void* y, int M, int F, void* stream) {
  DADD_REQUIRE(x && y, "gelu: null pointer");
  DADD_REQUIRE(M > 0 && F > 0 && F % 8 == 0, "gelu: M=%d must be positive and F=%d a positive multiple of 8", M, F);
  DADD_REQUIRE(dadd_aligned16(x) && dadd_aligned16(y), "gelu: pointers must be 16-byte aligned");
  const size_t nvec = (size_t)M * (F / 8);
  DADD_REQUIRE((nvec + 255) / 256 <= 0x7fffffffu, "gelu: too many elements");
  dadd_launch({DADD_KNAME("gelu_kernel"), 0.0, (double)M * F * 4.0}, gelu_kernel, dim3((unsigned)((nvec + 255) / 256)),
              dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const half_t*>(x), static_cast<half_t*>(y), nvec);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}

extern "C" int dadd_gelu_grad_f16(const void* x, const void* dy, void* dx, int M, int F, void* stream) {
  DADD_REQUIRE(x && dy && dx, "gelu_grad: null pointer");
  DADD_REQUIRE(M > 0 && F > 0 && F % 8 == 0, "gelu_grad: M=%d must be positive and F=%d a positive multiple of 8", M, F);
  DADD_REQUIRE(dadd_aligned16(x) && dadd_aligned16(dy) && dadd_aligned16(dx), "gelu_grad: pointers must be 16-byte aligned");
  const size_t nvec = (size_t)M * (F / 8);
  DADD_REQUIRE((nvec + 255) / 256 <= 0x7fffffffu, "gelu_grad: too many elements");
  dadd_launch({DADD_KNAME("gelu_grad_kernel"), 0.0, (double)M * F * 6.0}, gelu_grad_kernel,
              dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
              static_cast<const half_t*>(x), static_cast<const half_t*>(dy), static_cast<half_t*>(dx), nvec);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}

extern "C" int dadd_purifier_gate_tail_f16(const void* img, const void* dis, const void* z, const float* gamma,
                                           const float* beta, float* out, int M, int C, float eps, void* stream) {
  DADD_REQUIRE(img && dis && z && gamma && beta && out, "purifier_gate_tail: null pointer");
  DADD_REQUIRE(gt_sizes_ok(M, C), "purifier_gate_tail: C=%d must be a multiple of 8 and <= %d, M=%d positive", C,
               8 * 64 * GT_MAXV, M);
  DADD_REQUIRE(dadd_aligned16(img) && dadd_aligned16(dis) && dadd_aligned16(z) && dadd_aligned16(gamma) &&
                   dadd_aligned16(beta) && dadd_aligned16(out), "purifier_gate_tail: pointers must be 16-byte aligned");
  dadd_launch({DADD_KNAME("gate_tail_kernel"), 0.0, (double)M * C * 10.0}, gate_tail_kernel, dim3((M + 3) / 4), dim3(256), 0,
              static_cast<hipStream_t>(stream), static_cast<const half_t*>(img), static_cast<const half_t*>(dis),
              static_cast<const half_t*>(z), gamma, beta, out, M, C, eps);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}

extern "C" int dadd_purifier_gate_tail_grad_f16(const void* img, const void* dis, const void* z, const float* dout,
                                                const float* gamma, void* dimg, void* ddis, void* dz, float* dgamma,
                                                float* dbeta, float* ws, int M, int C, float eps, void* stream) {
  DADD_REQUIRE(img && dis && z && dout && gamma, "purifier_gate_tail_grad: null pointer");
  DADD_REQUIRE(gt_sizes_ok(M, C), "purifier_gate_tail_grad: C=%d must be a multiple of 8 and <= %d, M=%d positive", C,
               8 * 64 * GT_MAXV, M);
  DADD_REQUIRE((dgamma != nullptr) == (dbeta != nullptr), "purifier_gate_tail_grad: dgamma and dbeta come together");
  DADD_REQUIRE(dimg || ddis || dz || dgamma, "purifier_gate_tail_grad: no output");
  DADD_REQUIRE(!dgamma || ws, "purifier_gate_tail_grad: dgamma / dbeta need ws");
  DADD_REQUIRE(dadd_aligned16(img) && dadd_aligned16(dis) && dadd_aligned16(z) && dadd_aligned16(dout) &&
                   dadd_aligned16(gamma) && dadd_aligned16(dimg) && dadd_aligned16(ddis) && dadd_aligned16(dz) &&
                   (((uintptr_t)ws) & 7) == 0, "purifier_gate_tail_grad: pointers must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nblk = dadd_row_wave_blocks(M);
  float* part = dgamma ? ws : nullptr;
  const int nout = (dimg != nullptr) + (ddis != nullptr) + (dz != nullptr);
  dadd_launch({DADD_KNAME("gate_tail_grad_kernel"), 0.0, (double)M * C * (10.0 + 2.0 * nout)}, gate_tail_grad_kernel, dim3(nblk),
              dim3(256), (unsigned)((size_t)2 * C * sizeof(float)), s, static_cast<const half_t*>(img),
              static_cast<const half_t*>(dis), static_cast<const half_t*>(z), dout, gamma, static_cast<half_t*>(dimg),
              static_cast<half_t*>(ddis), static_cast<half_t*>(dz), part, M, C, eps);
  DADD_LAUNCH_CHECK();
  return dgamma ? dadd_norm_grad_finish(ws, dgamma, dbeta, nblk, C, s) : DADD_OK;
}
