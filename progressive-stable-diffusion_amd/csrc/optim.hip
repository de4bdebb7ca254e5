// The optimizer of a training step (include/dadd_hip_optim.h): gradient statistics, the scalar work of clipping / loss
// scale / bias correction in one workgroup, and the fused AdamW pass that also writes the EMA, the 16-bit working copy
// and the zeroed gradient.  Pure streaming: 16-byte loads and stores, no LDS beyond the reduction, no atomics.
#include "dadd_common.h"
#include "../../include/dadd_hip_optim.h"

#include <limits.h>

// Every operation of the update is rounded to fp32 on its own (the order is the contract the tests restate on the
// CPU): hipcc contracts a * b + c into an fma by default, so switch that off for this file.
#pragma clang fp contract(off)

namespace {

constexpr int OPT_CHUNK = DADD_OPTIM_CHUNK;
constexpr int OPT_BLOCK = 256;
constexpr int OPT_NV = OPT_CHUNK / (4 * OPT_BLOCK);   // 16-byte vectors per lane, array and chunk
constexpr int OPT_DEFAULT_BLOCKS = 2048;              // 8 workgroups of 4 waves per CU on 256 CUs
static_assert(OPT_NV == 4, "the summation depth documented in the header assumes 16 values per lane");

__device__ __forceinline__ bool opt_nonfinite(float x) {
  return (__builtin_bit_cast(unsigned, x) & 0x7f800000u) == 0x7f800000u;
}

__global__ __launch_bounds__(OPT_BLOCK) void optim_grad_stats_kernel(const float* __restrict__ g, float* __restrict__ partials,
                                                                     int* __restrict__ flags, int n_chunks) {
  __shared__ float s_sum[OPT_BLOCK / DADD_WAVE];
  __shared__ int s_bad[OPT_BLOCK / DADD_WAVE];
  const int tid = threadIdx.x, wave = tid / DADD_WAVE, lane = tid % DADD_WAVE;
  for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const f4* src = reinterpret_cast<const f4*>(g + (size_t)chunk * OPT_CHUNK);
    f4 x[OPT_NV];
#pragma unroll
    for (int j = 0; j < OPT_NV; ++j) x[j] = src[j * OPT_BLOCK + tid];
    float sum = 0.0f;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < OPT_NV; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = x[j][e];
        bad = bad || opt_nonfinite(t);
        const float sq = t * t;
        sum = (j == 0 && e == 0) ? sq : sum + sq;
      }
    sum = wave_sum(sum);
    const int wbad = __any(bad);
    if (lane == 0) {
      s_sum[wave] = sum;
      s_bad[wave] = wbad;
    }
    __syncthreads();
    if (tid == 0) {
      partials[chunk] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
      flags[chunk] = (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) ? 1 : 0;
    }
    __syncthreads();
  }
}

// One workgroup of OPT_FIN_BLOCK lanes.  Lane l adds partials l, l + OPT_FIN_BLOCK, ... in that order in double, OPT_FIN_UNROLL
// independent loads in flight per lane and array (one dependent load per iteration ran at 5 GB/s: 350 us for the 225 k
// chunks of the full model); then a fixed tree over the lanes.
constexpr int OPT_FIN_BLOCK = 1024;
constexpr int OPT_FIN_UNROLL = 8;

__global__ __launch_bounds__(OPT_FIN_BLOCK) void optim_finalize_kernel(const float* __restrict__ partials,
                                                                       const int* __restrict__ flags, int n_chunks,
                                                                       dadd_optim_state* __restrict__ st) {
  __shared__ double s_sum[OPT_FIN_BLOCK];
  __shared__ int s_bad[OPT_FIN_BLOCK];
  const int tid = threadIdx.x;
  double sum = 0.0;
  int bad = 0;
  constexpr int SPAN = OPT_FIN_BLOCK * OPT_FIN_UNROLL;
  const int n_full = n_chunks - n_chunks % SPAN;
  for (int base = 0; base < n_full; base += SPAN) {
    float x[OPT_FIN_UNROLL];
    int f[OPT_FIN_UNROLL];
#pragma unroll
    for (int u = 0; u < OPT_FIN_UNROLL; ++u) {
      x[u] = partials[base + u * OPT_FIN_BLOCK + tid];
      f[u] = flags[base + u * OPT_FIN_BLOCK + tid];
    }
#pragma unroll
    for (int u = 0; u < OPT_FIN_UNROLL; ++u) {
      sum += (double)x[u];
      bad |= f[u];
    }
  }
  for (int i = n_full + tid; i < n_chunks; i += OPT_FIN_BLOCK) {
    sum += (double)partials[i];
    bad |= flags[i];
  }
  s_sum[tid] = sum;
  s_bad[tid] = bad;
  __syncthreads();
  for (int w = OPT_FIN_BLOCK / 2; w > 0; w >>= 1) {
    if (tid < w) {
      s_sum[tid] += s_sum[tid + w];
      s_bad[tid] |= s_bad[tid + w];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const bool found_inf = s_bad[0] != 0;
  const float scale = st->scale;
  const double inv_scale = scale == 0.0f ? 1.0 : 1.0 / (double)scale;
  const double norm = sqrt(s_sum[0]) * inv_scale;
  const float max_norm = st->max_norm;
  double coef = inv_scale;
  if (max_norm > 0.0f) coef *= fmin(1.0, (double)max_norm / (norm + 1e-6));
  st->found_inf = found_inf ? 1 : 0;
  st->grad_norm = (float)norm;
  st->coef = found_inf ? 0.0f : (float)coef;
  if (!found_inf) {
    const int t = st->step + 1;
    st->step = t;
    int ng = st->n_groups;
    ng = ng < 0 ? 0 : (ng > DADD_OPTIM_MAX_GROUPS ? DADD_OPTIM_MAX_GROUPS : ng);
    for (int k = 0; k < ng; ++k) {
      dadd_optim_group* gr = &st->group[k];
      const double lr = (double)st->lr[k];
      gr->decay = (float)(1.0 - lr * (double)gr->weight_decay);
      gr->step_size = (float)(lr / (1.0 - pow(1.0 - (double)gr->one_minus_beta1, (double)t)));
      gr->rsqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow(1.0 - (double)gr->one_minus_beta2, (double)t)));
    }
  }
  if (scale != 0.0f) {
    if (found_inf) {
      st->scale = scale * st->backoff_factor;
      st->growth_tracker = 0;
    } else {
      const int tr = st->growth_tracker + 1;
      if (tr >= st->growth_interval) {
        st->scale = scale * st->growth_factor;
        st->growth_tracker = 0;
      } else {
        st->growth_tracker = tr;
      }
    }
  }
}

struct OptStepArgs {
  float* p;
  float* g;
  float* m;
  float* v;
  float* ema;
  void* p16;
  const dadd_optim_state* state;
  int chunk_end[DADD_OPTIM_MAX_GROUPS];   // first chunk past group k; INT_MAX behind the last group
  int n_chunks;
  float ema_weight;
};

template <typename T16>
__device__ __forceinline__ void opt_store16(void* p16, size_t vec, f4 x) {
  typedef T16 t4 __attribute__((ext_vector_type(4)));
  t4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (T16)x[e];
  reinterpret_cast<t4*>(p16)[vec] = o;
}

// P16: 0 no working copy, 1 fp16, 2 bf16
template <int P16, bool EMA, bool ZERO>
__global__ __launch_bounds__(OPT_BLOCK) void optim_adamw_step_kernel(const OptStepArgs a) {
  const dadd_optim_state* __restrict__ st = a.state;
  const bool skip = st->found_inf != 0;
  const float c = st->coef;
  const int tid = threadIdx.x;
  for (int chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
    const size_t v0 = (size_t)chunk * (OPT_CHUNK / 4);   // index of the chunk's first 16-byte vector
    f4* P = reinterpret_cast<f4*>(a.p) + v0;
    f4* G = reinterpret_cast<f4*>(a.g) + v0;
    f4 pv[OPT_NV];
    if (!skip) {
      int k = 0;
#pragma unroll
      for (int i = 0; i < DADD_OPTIM_MAX_GROUPS - 1; ++i) k += chunk >= a.chunk_end[i] ? 1 : 0;
      const dadd_optim_group* gr = &st->group[k];
      const float beta2 = gr->beta2, eps = gr->eps, omb1 = gr->one_minus_beta1, omb2 = gr->one_minus_beta2;
      const float decay = gr->decay, step_size = gr->step_size, rsqrt_bc2 = gr->rsqrt_bc2;
      f4* M = reinterpret_cast<f4*>(a.m) + v0;
      f4* V = reinterpret_cast<f4*>(a.v) + v0;
      f4 gv[OPT_NV], mv[OPT_NV], vv[OPT_NV];
#pragma unroll
      for (int j = 0; j < OPT_NV; ++j) {
        pv[j] = P[j * OPT_BLOCK + tid];
        gv[j] = G[j * OPT_BLOCK + tid];
        mv[j] = M[j * OPT_BLOCK + tid];
        vv[j] = V[j * OPT_BLOCK + tid];
      }
#pragma unroll
      for (int j = 0; j < OPT_NV; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float gs = gv[j][e] * c;
          float pe = pv[j][e] * decay;
          const float me = mv[j][e] + (gs - mv[j][e]) * omb1;
          const float ve = vv[j][e] * beta2 + (gs * gs) * omb2;
          const float denom = sqrtf(ve) * rsqrt_bc2 + eps;
          pe = pe - step_size * (me / denom);
          pv[j][e] = pe;
          mv[j][e] = me;
          vv[j][e] = ve;
        }
        P[j * OPT_BLOCK + tid] = pv[j];
        M[j * OPT_BLOCK + tid] = mv[j];
        V[j * OPT_BLOCK + tid] = vv[j];
      }
    } else if (EMA || P16 != 0) {
#pragma unroll
      for (int j = 0; j < OPT_NV; ++j) pv[j] = P[j * OPT_BLOCK + tid];
    }
    if (EMA) {
      f4* E = reinterpret_cast<f4*>(a.ema) + v0;
      f4 ev[OPT_NV];
#pragma unroll
      for (int j = 0; j < OPT_NV; ++j) ev[j] = E[j * OPT_BLOCK + tid];
#pragma unroll
      for (int j = 0; j < OPT_NV; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) ev[j][e] = ev[j][e] + (pv[j][e] - ev[j][e]) * a.ema_weight;
        E[j * OPT_BLOCK + tid] = ev[j];
      }
    }
    if (P16 == 1) {
#pragma unroll
      for (int j = 0; j < OPT_NV; ++j) opt_store16<_Float16>(a.p16, v0 + j * OPT_BLOCK + tid, pv[j]);
    } else if (P16 == 2) {
#pragma unroll
      for (int j = 0; j < OPT_NV; ++j) opt_store16<__bf16>(a.p16, v0 + j * OPT_BLOCK + tid, pv[j]);
    }
    if (ZERO) {
      const f4 z = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int j = 0; j < OPT_NV; ++j) G[j * OPT_BLOCK + tid] = z;
    }
  }
}

template <int P16, bool EMA>
void opt_launch_step(bool zero, const OptStepArgs& a, int grid, double bytes, hipStream_t s) {
  if (zero)
    dadd_launch({"optim_adamw_step_kernel", 0.0, bytes}, optim_adamw_step_kernel<P16, EMA, true>, dim3(grid), dim3(OPT_BLOCK), 0,
                s, a);
  else
    dadd_launch({"optim_adamw_step_kernel", 0.0, bytes}, optim_adamw_step_kernel<P16, EMA, false>, dim3(grid), dim3(OPT_BLOCK), 0,
                s, a);
}

template <int P16>
void opt_launch_step(bool ema, bool zero, const OptStepArgs& a, int grid, double bytes, hipStream_t s) {
  if (ema)
    opt_launch_step<P16, true>(zero, a, grid, bytes, s);
  else
    opt_launch_step<P16, false>(zero, a, grid, bytes, s);
}

int opt_grid(long long n_chunks, int max_blocks) {
  const long long cap = max_blocks > 0 ? max_blocks : OPT_DEFAULT_BLOCKS;
  return (int)(n_chunks < cap ? n_chunks : cap);
}

}  // namespace

extern "C" int dadd_optim_grad_stats(const float* g, long long n, float* partials, int* flags, int max_blocks,
                                     void* stream) {
  DADD_REQUIRE(g && partials && flags, "optim_grad_stats: null pointer");
  DADD_REQUIRE(n > 0 && n % OPT_CHUNK == 0, "optim_grad_stats: n=%lld must be a positive multiple of %d", n, OPT_CHUNK);
  DADD_REQUIRE(n / OPT_CHUNK <= INT_MAX, "optim_grad_stats: n=%lld has too many chunks", n);
  DADD_REQUIRE(max_blocks >= 0, "optim_grad_stats: max_blocks=%d must not be negative", max_blocks);
  DADD_REQUIRE(dadd_aligned16(g), "optim_grad_stats: g must be 16-byte aligned");
  DADD_REQUIRE((((uintptr_t)partials) & 3) == 0 && (((uintptr_t)flags) & 3) == 0, "optim_grad_stats: misaligned scratch");
  const int n_chunks = (int)(n / OPT_CHUNK);
  dadd_launch({"optim_grad_stats_kernel", 0.0, (double)n * 4.0}, optim_grad_stats_kernel, dim3(opt_grid(n_chunks, max_blocks)),
              dim3(OPT_BLOCK), 0, static_cast<hipStream_t>(stream), g, partials, flags, n_chunks);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}

extern "C" int dadd_optim_finalize(const float* partials, const int* flags, long long n_chunks, dadd_optim_state* state,
                                   void* stream) {
  DADD_REQUIRE(partials && flags && state, "optim_finalize: null pointer");
  DADD_REQUIRE(n_chunks > 0 && n_chunks <= INT_MAX, "optim_finalize: n_chunks=%lld out of range", n_chunks);
  DADD_REQUIRE((((uintptr_t)partials) & 3) == 0 && (((uintptr_t)flags) & 3) == 0 && (((uintptr_t)state) & 3) == 0,
               "optim_finalize: misaligned pointer");
  dadd_launch({"optim_finalize_kernel", 0.0, (double)n_chunks * 8.0}, optim_finalize_kernel, dim3(1), dim3(OPT_FIN_BLOCK), 0,
              static_cast<hipStream_t>(stream), partials, flags, (int)n_chunks, state);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}

extern "C" int dadd_optim_adamw_step(float* p, float* g, float* m, float* v, float* ema, void* p16, long long n,
                                     const int* group_chunks, int n_groups, const dadd_optim_state* state,
                                     float ema_weight, int flags, int max_blocks, void* stream) {
  DADD_REQUIRE(p && g && m && v && group_chunks && state, "optim_adamw_step: null pointer");
  DADD_REQUIRE(n > 0 && n % OPT_CHUNK == 0, "optim_adamw_step: n=%lld must be a positive multiple of %d", n, OPT_CHUNK);
  DADD_REQUIRE(n / OPT_CHUNK <= INT_MAX, "optim_adamw_step: n=%lld has too many chunks", n);
  DADD_REQUIRE(max_blocks >= 0, "optim_adamw_step: max_blocks=%d must not be negative", max_blocks);
  DADD_REQUIRE((flags & ~(DADD_OPTIM_EMA | DADD_OPTIM_P16_F16 | DADD_OPTIM_P16_BF16 | DADD_OPTIM_ZERO_GRAD)) == 0,
               "optim_adamw_step: unknown flags 0x%x", flags);
  const bool want_ema = (flags & DADD_OPTIM_EMA) != 0;
  const int p16_kind = (flags & DADD_OPTIM_P16_F16) ? 1 : (flags & DADD_OPTIM_P16_BF16) ? 2 : 0;
  DADD_REQUIRE(!((flags & DADD_OPTIM_P16_F16) && (flags & DADD_OPTIM_P16_BF16)),
               "optim_adamw_step: the working copy is fp16 or bf16, not both");
  DADD_REQUIRE(want_ema == (ema != nullptr), "optim_adamw_step: ema goes with DADD_OPTIM_EMA");
  DADD_REQUIRE((p16_kind != 0) == (p16 != nullptr), "optim_adamw_step: p16 goes with a DADD_OPTIM_P16 flag");
  DADD_REQUIRE(dadd_aligned16(p) && dadd_aligned16(g) && dadd_aligned16(m) && dadd_aligned16(v) && dadd_aligned16(ema) &&
                   (((uintptr_t)p16) & 7) == 0 && (((uintptr_t)state) & 3) == 0,
               "optim_adamw_step: arrays must be 16-byte aligned (p16: 8-byte)");
  DADD_REQUIRE(n_groups >= 1 && n_groups <= DADD_OPTIM_MAX_GROUPS, "optim_adamw_step: n_groups=%d out of range", n_groups);
  const int n_chunks = (int)(n / OPT_CHUNK);
  OptStepArgs a;
  long long end = 0;
  for (int k = 0; k < DADD_OPTIM_MAX_GROUPS; ++k) {
    if (k < n_groups) {
      DADD_REQUIRE(group_chunks[k] >= 0, "optim_adamw_step: group %d has %d chunks", k, group_chunks[k]);
      end += group_chunks[k];
      DADD_REQUIRE(end <= n_chunks, "optim_adamw_step: the groups hold more than the arena's %d chunks", n_chunks);
    }
    a.chunk_end[k] = k < n_groups - 1 ? (int)end : INT_MAX;
  }
  DADD_REQUIRE(end == n_chunks, "optim_adamw_step: the groups hold %lld chunks, the arena %d", end, n_chunks);
  a.p = p; a.g = g; a.m = m; a.v = v; a.ema = ema; a.p16 = p16; a.state = state;
  a.n_chunks = n_chunks;
  a.ema_weight = ema_weight;
  const bool zero = (flags & DADD_OPTIM_ZERO_GRAD) != 0;
  const double bytes = (double)n * (28.0 + (want_ema ? 8.0 : 0.0) + (p16_kind ? 2.0 : 0.0) + (zero ? 4.0 : 0.0));
  const int grid = opt_grid(n_chunks, max_blocks);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (p16_kind == 1)
    opt_launch_step<1>(want_ema, zero, a, grid, bytes, s);
  else if (p16_kind == 2)
    opt_launch_step<2>(want_ema, zero, a, grid, bytes, s);
  else
    opt_launch_step<0>(want_ema, zero, a, grid, bytes, s);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}
