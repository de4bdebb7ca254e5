// Backward of the fp32 row path (include/dadd_hip_rows_grad.h): the gradients of linear_rows (AOE projector, time-embedding
// MLP, the concatenated time_emb_proj layers), of the AOE class interpolation and of the row that EPI_ROWVEC adds in a conv
// epilogue.  Traffic-bound kernels in the manner of cond_grad.hip: wave64, 16-byte loads / stores, fp32 arithmetic on the
// vector unit, per-workgroup partial sums added in workgroup order by a second launch, no atomics: results are
// bit-reproducible run to run.  Only the 16-bit kernels of rowvec_grad compile a second time in the bf16 twin.
#include "dadd_common.h"
#include "../../include/dadd_hip_rows_grad.h"

namespace {

#ifndef DADD_BF16
// ---- linear_rows backward ---------------------------------------------------------------------------------------------
// Grid (strip of `ns` rows of w) x (512-wide tile of K).  A lane owns one 8-wide chunk of K for the whole kernel: it keeps
// a = act_in(x) of the pass's 8 rows of x (64 registers) and the pass's dx sums over the rows of w its wave visits (64
// registers); a wave visits the rows n0 + wave, n0 + wave + 4, ... of the strip, one at a time: the row's 8 weights and
// its 8 dw sums are registers, the 8 dy values come from LDS as two 16-byte broadcasts.  dw[n][chunk] leaves with 16-byte
// stores; the four waves' dx sums are added in wave order through LDS and leave as the strip's partial part[strip][m][k].
constexpr int RG_KT = 512;       // K-tile: 64 lanes x 8
constexpr int RG_NS_MAX = 64;    // rows of w per strip: 64 x 512 fp32 = 128 KB, what later passes re-read from L2
constexpr int RG_MP = 8;         // rows of x per pass

// a = act_in(x) for dw.  The GELU takes Phi from libm's complementary error function: 1 + erff(v / sqrt 2) cancels for
// v < 0 (at v = -3 it keeps 2e-5 of Phi, twenty times the bound of a one-term dw), erfcf(-v / sqrt 2) keeps Phi's own bits.
__device__ __forceinline__ float rg_act(float v, int act) {
  return act == 1 ? dadd_silu(v) : (act == 2 ? 0.5f * v * erfcf(-v * 0.70710678118654752440f) : v);
}
// act_in'(x), evaluated in double and rounded once.  Both derivatives have a zero (SiLU' at x = -1.278, GELU' at
// x = -0.752) next to which an fp32 evaluation keeps an absolute 3e-8 and no relative accuracy, while the bound of dx is
// relative to |act_in'(x)|: measured 2.5 times the bound at M x K = 8 x 520 with fp32 erfcf / expf.  The finish kernel
// evaluates M * K of them per call, so the double arithmetic is not on any hot path.
__device__ __forceinline__ float rg_act_grad(float xf, int act) {
  const double x = (double)xf;
  if (act == 1) {
    const double s = 1.0 / (1.0 + exp(-x));
    return (float)(s * (1.0 + x * (1.0 - s)));
  }
  if (act == 2) {
    const double Phi = 0.5 * erfc(-x * 0.70710678118654752440);
    const double phi = 0.39894228040143267794 * exp(-0.5 * x * x);
    return (float)(Phi + x * phi);
  }
  return 1.0f;
}

// DX: the partial sums of dx go to `part`; DW: dw (and db when not NULL) are written.  Without DX w is not read.
template <typename WT, bool DX, bool DW>
__global__ __launch_bounds__(256) void rows_grad_kernel(const float* __restrict__ x, const WT* __restrict__ w,
                                                        const float* __restrict__ dy, float* __restrict__ dw,
                                                        float* __restrict__ db, float* __restrict__ part, int M, int K,
                                                        int N, int act_in, int ns) {
  __shared__ __attribute__((aligned(16))) float dys[RG_NS_MAX * RG_MP];   // [row of the strip][row of the pass]
  __shared__ __attribute__((aligned(16))) float red[RG_MP * RG_KT];       // [row of the pass][k of the tile]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * ns;
  const int k0 = blockIdx.y * RG_KT + lane * 8;
  const bool active = k0 < K;            // K is a multiple of 8: a chunk is whole or absent
  const bool lead = blockIdx.y == 0;     // the K-tile that also writes db
  for (int m0 = 0; m0 < M; m0 += RG_MP) {
    const int mr = min(RG_MP, M - m0);
    for (int i = threadIdx.x; i < ns * RG_MP; i += 256) {
      const int r = i / ns, nl = i - r * ns;
      dys[nl * RG_MP + r] = (r < mr && n0 + nl < N) ? dy[(size_t)(m0 + r) * N + n0 + nl] : 0.f;
    }
    float a[RG_MP][8], dxa[RG_MP][8];
#pragma unroll
    for (int r = 0; r < RG_MP; ++r) {
#pragma unroll
      for (int c = 0; c < 8; ++c) a[r][c] = dxa[r][c] = 0.f;
      if (DW && active && r < mr) {
        dadd_load8(x + (size_t)(m0 + r) * K + k0, a[r]);
#pragma unroll
        for (int c = 0; c < 8; ++c) a[r][c] = rg_act(a[r][c], act_in);
      }
    }
    __syncthreads();
    for (int nl = wave; nl < ns; nl += 4) {
      const int n = n0 + nl;
      if (n >= N) break;               // (a whole wave)
      float wv[8], dwv[8], dyr[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) wv[c] = dwv[c] = 0.f;
      if (DX && active) dadd_load8(w + (size_t)n * K + k0, wv);
      dadd_load8(dys + nl * RG_MP, dyr);
#pragma unroll
      for (int r = 0; r < RG_MP; ++r) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          if (DW) dwv[c] = fmaf(dyr[r], a[r][c], dwv[c]);
          if (DX) dxa[r][c] = fmaf(dyr[r], wv[c], dxa[r][c]);
        }
      }
      if (DW && active) {
        float* o = dw + (size_t)n * K + k0;
        if (m0 > 0) {                  // this lane stored the sum of the earlier passes itself
          float prev[8];
          dadd_load8(o, prev);
#pragma unroll
          for (int c = 0; c < 8; ++c) dwv[c] += prev[c];
        }
        dadd_store8(o, dwv);
      }
      if (DW && db != nullptr && lead && lane == 0) {
        float s = dyr[0];
#pragma unroll
        for (int r = 1; r < RG_MP; ++r) s += dyr[r];
        db[n] = m0 > 0 ? db[n] + s : s;
      }
    }
    if (DX) {
      for (int v = 0; v < 4; ++v) {
        if (wave == v) {
#pragma unroll
          for (int r = 0; r < RG_MP; ++r) {
            float* s = red + r * RG_KT + lane * 8;
            if (v > 0) {
              float prev[8];
              dadd_load8(s, prev);
#pragma unroll
              for (int c = 0; c < 8; ++c) dxa[r][c] += prev[c];
            }
            dadd_store8(s, dxa[r]);
          }
        }
        __syncthreads();
      }
      if (active) {
        for (int r = wave; r < mr; r += 4) {
          float v8[8];
          dadd_load8(red + r * RG_KT + lane * 8, v8);
          dadd_store8(part + ((size_t)blockIdx.x * M + m0 + r) * K + k0, v8);
        }
      }
    }
    __syncthreads();     // dys and red are rewritten by the next pass
  }
}

// dx[i] = act_in'(x[i]) * sum over the strips of part[strip][i], i over M * K in 4-wide columns.  A block takes 32 columns;
// thread (q, column) adds the strips q, q + 8, ..., the eight slices are then added in slice order.
__global__ __launch_bounds__(256) void rows_grad_finish_kernel(const float* __restrict__ part, const float* __restrict__ x,
                                                               float* __restrict__ dx, int nstrip, size_t mk, int act_in) {
  __shared__ f4 red[8][32];
  const int t = threadIdx.x, col = t & 31, q = t >> 5;
  const size_t i = ((size_t)blockIdx.x * 32 + col) * 4;
  f4 s = {0.f, 0.f, 0.f, 0.f};
  if (i < mk) {
    for (int k = q; k < nstrip; k += 8) s += *reinterpret_cast<const f4*>(part + (size_t)k * mk + i);
  }
  red[q][col] = s;
  __syncthreads();
  if (t < 32 && i < mk) {
    s = red[0][col];
#pragma unroll
    for (int k = 1; k < 8; ++k) s += red[k][col];
    if (act_in != 0) {
      const f4 xv = *reinterpret_cast<const f4*>(x + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] *= rg_act_grad(xv[e], act_in);
    }
    *reinterpret_cast<f4*>(dx + i) = s;
  }
}

// ---- AOE class interpolation backward: one thread per column, the class table's gradient in registers -----------------
constexpr int AOE_MAX_CLASSES = 16;

__global__ __launch_bounds__(256) void aoe_interp_grad_kernel(const float* __restrict__ labels,
                                                              const float* __restrict__ dout, float* __restrict__ dbase,
                                                              float* __restrict__ ddeltas, int B, int D, int classes) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  float dt[AOE_MAX_CLASSES];
#pragma unroll
  for (int c = 0; c < AOE_MAX_CLASSES; ++c) dt[c] = 0.f;
  const float top = (float)(classes - 1);
  for (int b = 0; b < B; ++b) {
    const float y = fminf(fmaxf(labels[b], 0.f), top);        // aoe_interp_kernel's lo, hi, frac
    const float lo = floorf(y);
    const float frac = y - lo;
    const int lo_i = (int)lo, hi_i = min(lo_i + 1, classes - 1);
    const float g = dout[(size_t)b * D + d];
    const float glo = (1.0f - frac) * g, ghi = frac * g;
#pragma unroll
    for (int c = 0; c < AOE_MAX_CLASSES; ++c) {                // (no indexed register array: it would live in scratch)
      if (c == lo_i) dt[c] += glo;
      if (c == hi_i) dt[c] += ghi;
    }
  }
  float s = 0.f;
#pragma unroll
  for (int c = AOE_MAX_CLASSES - 1; c >= 1; --c) {             // suffix sums: the transpose of the table's cumsum
    if (c < classes) {
      s += dt[c];
      ddeltas[(size_t)(c - 1) * D + d] = s;
    }
  }
  dbase[d] = s + dt[0];
}

int rg_strip(int K, int N) {         // rows of w per strip: the widest that still fills the machine twice
  const int kt = (K + RG_KT - 1) / RG_KT;
  for (int ns = RG_NS_MAX; ns > 16; ns >>= 1) {
    if ((long long)((N + ns - 1) / ns) * kt >= 512) return ns;
  }
  return 16;
}

bool rg_sizes_ok(int M, int K, int N) { return M > 0 && N > 0 && K > 0 && K % 8 == 0 && K <= 2048; }

template <typename WT>
void rg_launch(const float* x, const void* w, const float* dy, float* dw, float* db, float* part, int M, int K, int N,
               int act_in, int ns, bool want_dx, bool want_dw, hipStream_t s) {
  const dim3 grid((N + ns - 1) / ns, (K + RG_KT - 1) / RG_KT);
  const double wbytes = (double)N * K * sizeof(WT);
  const WT* wt = static_cast<const WT*>(w);
  const char* name = sizeof(WT) == 4 ? "rows_grad_kernel<float>" : "rows_grad_kernel<_Float16>";
  const DaddLaunchTag tag = {name, (want_dx ? 2.0 : 0.0) * M * N * K + (want_dw ? 2.0 : 0.0) * M * N * K,
                             (want_dx ? wbytes : 0.0) + (want_dw ? (double)N * K * 4.0 : 0.0) + (double)M * (N + K) * 4.0};
  if (want_dx && want_dw)
    dadd_launch(tag, rows_grad_kernel<WT, true, true>, grid, dim3(256), 0, s, x, wt, dy, dw, db, part, M, K, N, act_in, ns);
  else if (want_dx)
    dadd_launch(tag, rows_grad_kernel<WT, true, false>, grid, dim3(256), 0, s, x, wt, dy, dw, db, part, M, K, N, act_in, ns);
  else
    dadd_launch(tag, rows_grad_kernel<WT, false, true>, grid, dim3(256), 0, s, x, wt, dy, dw, db, part, M, K, N, act_in, ns);
}
#endif  // !DADD_BF16

// ---- gradient of the EPI_ROWVEC row: column sums of 16-bit NHWC dy per sample ----------------------------------------------
// Grid (512-channel tile, chunk of 64 pixels, sample).  Thread (lane, g) adds the pixels g, g + 4, ... of the chunk for its
// 8 channels; the four groups are added in group order through LDS; the block writes part[b][chunk][C].
constexpr int RV_ROWS = 64;

__global__ __launch_bounds__(256) void rowvec_grad_kernel(const half_t* __restrict__ dy, float* __restrict__ part, int HW,
                                                          int C) {
  __shared__ __attribute__((aligned(16))) float sm[512];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int v = blockIdx.x * 64 + lane;
  const bool active = v < (C >> 3);
  const int b = blockIdx.z, chunk = blockIdx.y;
  const int p0 = chunk * RV_ROWS, p1 = min(HW, p0 + RV_ROWS);
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  if (active) {
    for (int p = p0 + g; p < p1; p += 4) {
      const h8 d = *reinterpret_cast<const h8*>(dy + ((size_t)b * HW + p) * C + v * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += (float)d[e];
    }
  }
  for (int k = 0; k < 4; ++k) {
    if (g == k) {
#pragma unroll
      for (int e = 0; e < 8; ++e) sm[lane * 8 + e] = k == 0 ? acc[e] : sm[lane * 8 + e] + acc[e];
    }
    __syncthreads();
  }
  if (g == 0 && active) {
    float* o = part + ((size_t)b * gridDim.y + chunk) * C + v * 8;
    *reinterpret_cast<f4*>(o) = *reinterpret_cast<const f4*>(sm + lane * 8);
    *reinterpret_cast<f4*>(o + 4) = *reinterpret_cast<const f4*>(sm + lane * 8 + 4);
  }
}

// drow[b][c] = sum over the chunks of part[b][chunk][c], in chunk order
__global__ __launch_bounds__(256) void rowvec_grad_finish_kernel(const float* __restrict__ part, float* __restrict__ drow,
                                                                 int nchunk, int C, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int b = i / C, c = i - b * C;
  const float* p = part + (size_t)b * nchunk * C + c;
  float s = p[0];
#pragma unroll 8       // (eight loads in flight; the additions keep their order)
  for (int k = 1; k < nchunk; ++k) s += p[(size_t)k * C];
  drow[i] = s;
}

bool rv_sizes_ok(int B, int HW, int C) {
  return B > 0 && HW > 0 && C > 0 && C % 8 == 0 && B <= 65535 && HW <= RV_ROWS * 65535 &&
         (long long)B * C <= 0x7fffffffLL;
}

}  // namespace

#ifndef DADD_BF16
// host only, one copy for both storage types
extern "C" long long dadd_rowvec_grad_ws_floats(int B, int HW, int C) {
  if (!rv_sizes_ok(B, HW, C)) return -1;
  return (long long)B * ((HW + RV_ROWS - 1) / RV_ROWS) * C;
}

extern "C" long long dadd_linear_rows_grad_ws_floats(int M, int K, int N) {
  if (!rg_sizes_ok(M, K, N)) return -1;
  const int ns = rg_strip(K, N);
  return (long long)((N + ns - 1) / ns) * M * K;
}

extern "C" int dadd_linear_rows_grad_f32(const float* x, const void* w, const float* dy, float* dx, float* dw, float* db,
                                         float* ws, int M, int K, int N, int act_in, int w_f32, void* stream) {
  DADD_REQUIRE(x && w && dy, "linear_rows_grad: null pointer");
  DADD_REQUIRE(rg_sizes_ok(M, K, N), "linear_rows_grad: K=%d must be a multiple of 8 and <= 2048, M=%d and N=%d positive", K,
               M, N);
  DADD_REQUIRE(act_in >= 0 && act_in <= 2, "linear_rows_grad: act_in must be 0, 1 (SiLU) or 2 (GELU)");
  DADD_REQUIRE(dx || dw, "linear_rows_grad: no output");
  DADD_REQUIRE(dw || !db, "linear_rows_grad: db comes with dw");
  DADD_REQUIRE(!dx || ws, "linear_rows_grad: dx needs ws");
  DADD_REQUIRE(dadd_aligned16(x) && dadd_aligned16(w) && dadd_aligned16(dx) && dadd_aligned16(dw) && dadd_aligned16(ws),
               "linear_rows_grad: x, w, dx, dw and ws must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int ns = rg_strip(K, N);
  const int nstrip = (N + ns - 1) / ns;
  if (w_f32)
    rg_launch<float>(x, w, dy, dw, db, dx ? ws : nullptr, M, K, N, act_in, ns, dx != nullptr, dw != nullptr, s);
  else
    rg_launch<half_t>(x, w, dy, dw, db, dx ? ws : nullptr, M, K, N, act_in, ns, dx != nullptr, dw != nullptr, s);
  DADD_LAUNCH_CHECK();
  if (dx) {
    const size_t mk = (size_t)M * K;
    dadd_launch({"rows_grad_finish_kernel", 0.0, (double)(nstrip + 2) * mk * 4.0}, rows_grad_finish_kernel,
                dim3((unsigned)((mk / 4 + 31) / 32)), dim3(256), 0, s, (const float*)ws, x, dx, nstrip, mk, act_in);
    DADD_LAUNCH_CHECK();
  }
  return DADD_OK;
}

extern "C" int dadd_aoe_interp_grad_f32(const float* labels, const float* dout, float* dbase, float* ddeltas, int B, int D,
                                        int classes, void* stream) {
  DADD_REQUIRE(labels && dout && dbase && ddeltas, "aoe_interp_grad: null pointer");
  DADD_REQUIRE(B > 0 && D > 0 && classes >= 2 && classes <= AOE_MAX_CLASSES,
               "aoe_interp_grad: B=%d and D=%d must be positive and classes=%d in 2..%d", B, D, classes, AOE_MAX_CLASSES);
  dadd_launch({"aoe_interp_grad_kernel", 0.0, ((double)B + classes) * D * 4.0}, aoe_interp_grad_kernel, dim3((D + 255) / 256),
              dim3(256), 0, static_cast<hipStream_t>(stream), labels, dout, dbase, ddeltas, B, D, classes);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}
#endif  // !DADD_BF16

extern "C" int dadd_rowvec_grad_f16(const void* dy, float* drow, float* ws, int B, int HW, int C, void* stream) {
  DADD_REQUIRE(dy && drow && ws, "rowvec_grad: null pointer");
  DADD_REQUIRE(rv_sizes_ok(B, HW, C), "rowvec_grad: C=%d must be a multiple of 8, B=%d in 1..65535, HW=%d in 1..%d", C, B, HW,
               RV_ROWS * 65535);
  DADD_REQUIRE(dadd_aligned16(dy) && dadd_aligned16(drow) && dadd_aligned16(ws), "rowvec_grad: pointers must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nchunk = (HW + RV_ROWS - 1) / RV_ROWS;
  dadd_launch({DADD_KNAME("rowvec_grad_kernel"), 0.0, (double)B * HW * C * 2.0}, rowvec_grad_kernel,
              dim3(((C >> 3) + 63) / 64, nchunk, B), dim3(256), 0, s, static_cast<const half_t*>(dy), ws, HW, C);
  DADD_LAUNCH_CHECK();
  dadd_launch({DADD_KNAME("rowvec_grad_finish_kernel"), 0.0, (double)B * (nchunk + 1) * C * 4.0}, rowvec_grad_finish_kernel,
              dim3((B * C + 255) / 256), dim3(256), 0, s, (const float*)ws, drow, nchunk, C, B * C);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}
