// One-launch refresh of the packed weights of live inference plans from the fp32 masters (include/
// dadd_hip_plan_refresh.h): reads the optimizer's flat p (or its EMA), writes for every descriptor what the packers of
// engine.py produce for that tensor.  HBM-bound: one read of every master, one write of every packed weight.
//
// A workgroup of 256 lanes serves one unit of one descriptor:
//   16-bit kinds  1024 groups of 8 destination values.  Lane t takes groups t, t + 256, ..: one 16-byte store each, 8
//                 consecutive lanes write 128 contiguous bytes.  A group's 8 values are 8 consecutive fp32 of ONE source
//                 row in every kind (the permutations move rows or 16-byte chunks, never single values): two 16-byte
//                 loads.  UPSFOLD reads 1, 2 or 4 such runs (one per tap) and adds them in fp64.
//   fp32 kinds    2048 values, lane-strided 4-byte loads and stores (biases and norm vectors: odd offsets allowed).
//   LNFOLD        4 destination rows, one per wave.  Lane l walks the groups l, l + 64, .. of its row, keeps the two row
//                 sums in fp64 and hands them through a shuffle butterfly: no LDS, no barrier.
// Every rounding is the packer's: fp64 -> fp32 -> 16 bits, each to nearest even (torch converts float64 to a 16-bit type
// through fp32).  W * gamma is exact in fp64 (two 24-bit significands), so round32 of it is the fp32 product.
#include "dadd_common.h"
#include "../../include/dadd_hip_plan_refresh.h"

namespace {

constexpr int PR_STREAM_C = 320;
constexpr long long PR_HEAD_NUMEL = 40ll * 160 * 64;                             // 10 + 30 pieces of [160][64]
constexpr long long PR_FFN_CHUNK = 5ll * 128 * 64 + 2ll * 160 * 64;              // per 64 hidden channels
constexpr long long PR_FFN_NUMEL = 20 * PR_FFN_CHUNK + 10ll * 160 * 64;
constexpr int PR_FFN_ROWS = 2560;

__host__ __device__ inline bool pr_is_f32(int kind) {
  return kind == DADD_PLAN_REFRESH_COPY32 || kind == DADD_PLAN_REFRESH_GEGLU_B || kind == DADD_PLAN_REFRESH_FFN_BIAS;
}
__host__ __device__ inline bool pr_padded(int kind, int K, int Cs) { return kind == DADD_PLAN_REFRESH_CAST && Cs != K; }

// geglu_interleave: source row of destination row r, n2 = rows / 2
__host__ __device__ inline int pr_geglu_row(int r, int n2) {
  const int tile = r >> 7, wn = (r >> 6) & 1, q = r & 63;
  const int col = tile * 64 + wn * 32 + (q & 31);
  return q < 32 ? col : n2 + col;
}
// pack_ffn_stream: row of ff.net.0.proj behind row rr of the 128-row pieces of chunk ch: wave column wn -> [h0 g0 h1 g1]
__host__ __device__ inline int pr_ffn_row(int ch, int rr) {
  const int q = rr >> 4, e = rr & 15;
  return (q & 1) * 1280 + ch * 64 + (q >> 2) * 32 + ((q >> 1) & 1) * 16 + e;
}

// elements each destination receives (of its own type)
__host__ __device__ inline long long pr_dst_numel(int kind, int N, int K, int which) {
  if (which > 0) return kind == DADD_PLAN_REFRESH_LNFOLD ? N : 0;
  switch (kind) {
    case DADD_PLAN_REFRESH_COPY32:
    case DADD_PLAN_REFRESH_GEGLU_B: return N;
    case DADD_PLAN_REFRESH_FFN_BIAS: return PR_FFN_ROWS;
    case DADD_PLAN_REFRESH_UPSFOLD: return 16ll * N * K;
    case DADD_PLAN_REFRESH_HEAD_STREAM: return PR_HEAD_NUMEL;
    case DADD_PLAN_REFRESH_FFN_STREAM: return PR_FFN_NUMEL;
    default: return (long long)N * K;
  }
}
// elements read behind src_off[which]; 0 = that source is not used
__host__ __device__ inline long long pr_src_numel(int kind, int N, int K, int Cs, int which) {
  switch (kind) {
    case DADD_PLAN_REFRESH_COPY32:
    case DADD_PLAN_REFRESH_GEGLU_B: return which == 0 ? N : 0;
    case DADD_PLAN_REFRESH_CAST: return which == 0 ? (long long)N * Cs : 0;
    case DADD_PLAN_REFRESH_GEGLU_W: return which == 0 ? (long long)N * K : 0;
    case DADD_PLAN_REFRESH_LNFOLD: return which == 0 ? (long long)N * K : which == 3 ? N : K;
    case DADD_PLAN_REFRESH_UPSFOLD: return which == 0 ? 9ll * N * K : 0;
    case DADD_PLAN_REFRESH_HEAD_STREAM: return (long long)PR_STREAM_C * PR_STREAM_C;
    case DADD_PLAN_REFRESH_FFN_STREAM: return which == 0 ? (long long)PR_FFN_ROWS * PR_STREAM_C
                                            : which == 1 ? (long long)PR_STREAM_C * 1280
                                            : which == 2 ? (long long)PR_STREAM_C * PR_STREAM_C : 0;
    case DADD_PLAN_REFRESH_FFN_BIAS: return which == 0 ? PR_FFN_ROWS : 0;
  }
  return 0;
}
// units of work: fp32 values, groups of 8 (the padded CAST: rows), or LNFOLD rows
__host__ __device__ inline long long pr_units(int kind, int N, int K, int Cs) {
  if (pr_is_f32(kind)) return pr_dst_numel(kind, N, K, 0);
  if (kind == DADD_PLAN_REFRESH_LNFOLD || pr_padded(kind, K, Cs)) return N;
  return pr_dst_numel(kind, N, K, 0) / 8;
}
__host__ __device__ inline long long pr_wgs(int kind, int N, int K, int Cs) {
  const long long u = pr_units(kind, N, K, Cs);
  const int per = pr_is_f32(kind) ? DADD_PLAN_REFRESH_SCALARS
                  : kind == DADD_PLAN_REFRESH_LNFOLD ? DADD_PLAN_REFRESH_ROWS : DADD_PLAN_REFRESH_GROUPS;
  return (u + per - 1) / per;
}
// the contract of (kind, N, K, Cs, flags)
__host__ __device__ inline bool pr_shape_ok(int kind, int N, int K, int Cs, int flags) {
  if (kind < DADD_PLAN_REFRESH_COPY32 || kind > DADD_PLAN_REFRESH_FFN_BIAS || N <= 0) return false;
  if (flags & ~DADD_PLAN_REFRESH_GEGLU) return false;
  if (flags && kind != DADD_PLAN_REFRESH_LNFOLD) return false;
  switch (kind) {
    case DADD_PLAN_REFRESH_COPY32: return true;
    case DADD_PLAN_REFRESH_GEGLU_B: return N % 128 == 0;
    case DADD_PLAN_REFRESH_CAST:
      if (K <= 0) return false;
      return Cs == K ? ((long long)N * K) % 8 == 0 : (K == 8 && Cs >= 1 && Cs < 8);
    case DADD_PLAN_REFRESH_GEGLU_W: return K > 0 && K % 8 == 0 && N % 128 == 0;
    case DADD_PLAN_REFRESH_LNFOLD: return K > 0 && K % 8 == 0 && (!(flags & DADD_PLAN_REFRESH_GEGLU) || N % 128 == 0);
    case DADD_PLAN_REFRESH_UPSFOLD: return K > 0 && K % 8 == 0 && 16ll * N * K <= 0x7fffffffll * 8;
    default: return K == PR_STREAM_C;      // the streams and FFN_BIAS
  }
}
// everything the kernel can check of a descriptor: the contract, the source ranges, the room behind each destination,
// the alignment its vector accesses need
__host__ __device__ inline bool pr_fits(const dadd_plan_refresh_desc& d, long long src_numel) {
  if (!pr_shape_ok(d.kind, d.N, d.K, d.Cs, d.flags)) return false;
  const bool f32 = pr_is_f32(d.kind), vec = !f32 && !pr_padded(d.kind, d.K, d.Cs);
  for (int i = 0; i < 4; ++i) {
    const long long n = pr_src_numel(d.kind, d.N, d.K, d.Cs, i);
    if (n == 0) continue;
    if (d.kind == DADD_PLAN_REFRESH_LNFOLD && i == 3 && d.src_off[3] == -1) continue;       // no bias b
    if (d.src_off[i] < 0 || d.src_off[i] > src_numel - n) return false;
    if (vec && !(d.kind == DADD_PLAN_REFRESH_LNFOLD && i == 3) && (d.src_off[i] & 3)) return false;
  }
  for (int i = 0; i < 3; ++i) {
    const long long n = pr_dst_numel(d.kind, d.N, d.K, i);
    if (n == 0) continue;
    if (!d.dst[i] || d.dst_room[i] < n) return false;
    if (((uintptr_t)d.dst[i]) & ((i == 0 && !f32) ? 15 : 3)) return false;
  }
  return true;
}

// first fp32 element (from `src`) of the 8 consecutive values behind destination group g of a permutation kind
__device__ __forceinline__ long long pr_group_src(const dadd_plan_refresh_desc& d, long long g) {
  switch (d.kind) {
    case DADD_PLAN_REFRESH_GEGLU_W: {
      const int kg = d.K >> 3, r = (int)(g / kg), c8 = (int)(g % kg);
      return d.src_off[0] + (long long)pr_geglu_row(r, d.N >> 1) * d.K + c8 * 8;
    }
    case DADD_PLAN_REFRESH_HEAD_STREAM: {
      // piece = [160][64] LDS image: row r, 16-byte position p holds chunk p ^ ((r >> 1) & 7) (engine.lds_image)
      const int piece = (int)(g / 1280), w = (int)(g % 1280), r = w >> 3, chunk = (w & 7) ^ ((r >> 1) & 7);
      int row, which = 0;
      const int q = piece < 10 ? piece : piece - 10, kt = q % 5;
      row = (q / 5) * 160 + r;
      if (piece >= 10) {                  // to_q | to_k | to_v stacked by rows
        which = 1 + row / PR_STREAM_C;
        row %= PR_STREAM_C;
      }
      const long long base = which == 0 ? d.src_off[0] : which == 1 ? d.src_off[1] : which == 2 ? d.src_off[2] : d.src_off[3];
      return base + (long long)row * PR_STREAM_C + kt * 64 + chunk * 8;
    }
    case DADD_PLAN_REFRESH_FFN_STREAM: {
      const long long per = PR_FFN_CHUNK / 8;                       // 7680 groups per 64 hidden channels
      if (g < 20 * per) {
        const int ch = (int)(g / per);
        int w = (int)(g % per);
        if (w < 5 * 1024) {                                         // five [128][64] pieces of ff.net.0.proj
          const int kt = w >> 10, r = (w & 1023) >> 3, chunk = (w & 7) ^ ((r >> 1) & 7);
          return d.src_off[0] + (long long)pr_ffn_row(ch, r) * PR_STREAM_C + kt * 64 + chunk * 8;
        }
        w -= 5 * 1024;                                              // two [160][64] pieces of ff.net.2
        const int nh = w / 1280, r = (w % 1280) >> 3, chunk = (w & 7) ^ ((r >> 1) & 7);
        return d.src_off[1] + (long long)(nh * 160 + r) * 1280 + ch * 64 + chunk * 8;
      }
      const int q = (int)(g - 20 * per), piece = q / 1280, r = (q % 1280) >> 3, chunk = (q & 7) ^ ((r >> 1) & 7);
      return d.src_off[2] + (long long)((piece / 5) * 160 + r) * PR_STREAM_C + (piece % 5) * 64 + chunk * 8;
    }
    default: return d.src_off[0] + g * 8;                           // CAST
  }
}

// first tap and number of taps of S(parity, d): {0}, {1, 2} | {0, 1}, {2}
__device__ __forceinline__ void pr_ups_set(int parity, int dd, int& k0, int& cnt) {
  k0 = dd == 0 ? 0 : parity == 0 ? 1 : 2;
  cnt = parity != dd ? 2 : 1;
}

// A value that HAS been rounded to fp32, as far as the optimiser can tell: the packers round fp64 -> fp32 -> 16 bits, and
// without this the compiler merges the two steps into one rounding (fp32 multiply + conversion become v_fma_mixlo_f16
// under -ffp-contract=fast, fp64 -> fp32 -> fp16 one conversion), which lands on the other 16-bit neighbour near ties.
__device__ __forceinline__ float pr_round32(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

__device__ __forceinline__ double pr_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void plan_refresh_kernel(const float* __restrict__ src, long long src_numel,
                                                           const dadd_plan_refresh_desc* __restrict__ table, int n_desc) {
  const int tid = threadIdx.x;
  const int wg = blockIdx.x;
  int lo = 0, hi = n_desc - 1;           // the last descriptor whose wg0 is <= wg (uniform: scalar loads)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].wg0 <= wg) lo = mid; else hi = mid - 1;
  }
  const dadd_plan_refresh_desc& d = table[lo];      // read in place: uniform loads, no private copy
  const long long local = (long long)wg - d.wg0;
  // a table that does not fit the arrays (or a stale one) writes nothing
  if (!pr_fits(d, src_numel) || local < 0 || local >= pr_wgs(d.kind, d.N, d.K, d.Cs)) return;
  const int kind = d.kind, N = d.N, K = d.K;
  const long long units = pr_units(kind, N, K, d.Cs);

  if (pr_is_f32(kind)) {
    float* __restrict__ D = static_cast<float*>(d.dst[0]);
    const float* __restrict__ S = src + d.src_off[0];
#pragma unroll
    for (int i = 0; i < DADD_PLAN_REFRESH_SCALARS / 256; ++i) {
      const long long e = local * DADD_PLAN_REFRESH_SCALARS + i * 256 + tid;
      if (e < units) {
        const long long s = kind == DADD_PLAN_REFRESH_COPY32 ? e
                            : kind == DADD_PLAN_REFRESH_GEGLU_B ? pr_geglu_row((int)e, N >> 1)
                                                                : pr_ffn_row((int)e >> 7, (int)e & 127);
        D[e] = S[s];
      }
    }
    return;
  }

  if (kind == DADD_PLAN_REFRESH_LNFOLD) {
    const int lane = tid & 63;
    const long long r = local * DADD_PLAN_REFRESH_ROWS + (tid >> 6);
    if (r >= N) return;                  // (whole waves leave: the shuffles below see full waves)
    const int s = (d.flags & DADD_PLAN_REFRESH_GEGLU) ? pr_geglu_row((int)r, N >> 1) : (int)r;
    const float* __restrict__ W = src + d.src_off[0] + (long long)s * K;
    const float* __restrict__ G = src + d.src_off[1];
    const float* __restrict__ Bt = src + d.src_off[2];
    half_t* __restrict__ O = static_cast<half_t*>(d.dst[0]) + r * K;
    double c1 = 0.0, bias = 0.0;
    for (int k = lane * 8; k < K; k += 512) {
      float w[8], g[8], b[8];
      dadd_load8(W + k, w);
      dadd_load8(G + k, g);
      dadd_load8(Bt + k, b);
      h8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float p = pr_round32(w[e] * g[e]);         // = round32 of the exact fp64 product
        o[e] = (half_t)p;
        c1 += (double)(float)o[e];
        bias += (double)w[e] * (double)b[e];
      }
      *reinterpret_cast<h8*>(O + k) = o;
    }
    c1 = pr_wave_sum(c1);
    bias = pr_wave_sum(bias);
    if (lane == 0) {
      static_cast<float*>(d.dst[1])[r] = (float)c1;
      static_cast<float*>(d.dst[2])[r] = (float)(bias + (d.src_off[3] >= 0 ? (double)src[d.src_off[3] + s] : 0.0));
    }
    return;
  }

  half_t* __restrict__ D = static_cast<half_t*>(d.dst[0]);
#pragma unroll 1
  for (int i = 0; i < DADD_PLAN_REFRESH_GROUPS / 256; ++i) {
    const long long g = local * DADD_PLAN_REFRESH_GROUPS + i * 256 + tid;
    if (g >= units) break;
    h8 o;
    if (pr_padded(kind, K, d.Cs)) {      // one (n, tap) row of Cs < 8 values, zero-padded to 8
      const float* __restrict__ S = src + d.src_off[0] + g * d.Cs;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = e < d.Cs ? (half_t)S[e] : (half_t)0.0f;
    } else if (kind == DADD_PLAN_REFRESH_UPSFOLD) {
      const int kg = K >> 3, c8 = (int)(g % kg), t = (int)((g / kg) & 3);
      const long long nn = g / (4 * kg);
      const int n = (int)(nn % N), ph = (int)(nn / N);
      int ky0, nky, kx0, nkx;
      pr_ups_set(ph >> 1, t >> 1, ky0, nky);
      pr_ups_set(ph & 1, t & 1, kx0, nkx);
      const float* __restrict__ S = src + d.src_off[0] + (long long)n * 9 * K + c8 * 8;
      double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int ky = ky0; ky < ky0 + nky; ++ky)
        for (int kx = kx0; kx < kx0 + nkx; ++kx) {
          float w[8];
          dadd_load8(S + (long long)(3 * ky + kx) * K, w);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += (double)(float)(half_t)w[e];
        }
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (half_t)pr_round32((float)acc[e]);
    } else {
      float w[8];
      dadd_load8(src + pr_group_src(d, g), w);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (half_t)w[e];
    }
    *reinterpret_cast<h8*>(D + g * 8) = o;
  }
}

}  // namespace

#ifndef DADD_BF16   // host-only planning: one copy in the library
#include <algorithm>
#include <vector>

extern "C" long long dadd_plan_refresh_wgs(int kind, int N, int K, int Cs, int flags) {
  if (!pr_shape_ok(kind, N, K, Cs, flags)) return -1;
  return pr_wgs(kind, N, K, Cs);
}

extern "C" long long dadd_plan_refresh_plan(dadd_plan_refresh_desc* descs, int n, long long src_numel) {
  if (!descs || n <= 0 || src_numel <= 0) {
    dadd_set_error("plan_refresh_plan: null table, n=%d or src_numel=%lld not positive", n, src_numel);
    return -1;
  }
  struct Range { uintptr_t lo, hi; int desc; };
  std::vector<Range> ranges;
  long long wgs = 0;
  for (int i = 0; i < n; ++i) {
    dadd_plan_refresh_desc& d = descs[i];
    if (!pr_shape_ok(d.kind, d.N, d.K, d.Cs, d.flags)) {
      dadd_set_error("plan_refresh_plan: descriptor %d: kind %d, N %d, K %d, Cs %d, flags %d is outside the contract "
                     "(include/dadd_hip_plan_refresh.h)", i, d.kind, d.N, d.K, d.Cs, d.flags);
      return -1;
    }
    if (!pr_fits(d, src_numel)) {
      dadd_set_error("plan_refresh_plan: descriptor %d (kind %d, N %d, K %d): a source range [%lld | %lld | %lld | %lld] "
                     "leaves [0, %lld) or is misaligned (4 elements), or a destination is null, misaligned or has less "
                     "room (%lld, %lld, %lld) than the kind writes", i, d.kind, d.N, d.K, d.src_off[0], d.src_off[1],
                     d.src_off[2], d.src_off[3], src_numel, d.dst_room[0], d.dst_room[1], d.dst_room[2]);
      return -1;
    }
    for (int j = 0; j < 3; ++j) {
      const long long len = pr_dst_numel(d.kind, d.N, d.K, j);
      if (len == 0) continue;
      const uintptr_t lo = (uintptr_t)d.dst[j];
      ranges.push_back({lo, lo + (uintptr_t)len * ((j == 0 && !pr_is_f32(d.kind)) ? 2 : 4), i});
    }
    const long long t = pr_wgs(d.kind, d.N, d.K, d.Cs);
    if (wgs + t > 0x7fffffffll) {
      dadd_set_error("plan_refresh_plan: more than 2^31 - 1 workgroups");
      return -1;
    }
    d.wg0 = (int)wgs;
    d.reserved[0] = d.reserved[1] = 0;
    wgs += t;
  }
  std::sort(ranges.begin(), ranges.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
  for (size_t i = 1; i < ranges.size(); ++i)
    if (ranges[i].lo < ranges[i - 1].hi) {
      dadd_set_error("plan_refresh_plan: the destinations of descriptors %d and %d overlap", ranges[i - 1].desc,
                     ranges[i].desc);
      return -1;
    }
  return wgs;
}
#endif

extern "C" int dadd_plan_refresh_f16(const void* src, long long src_numel, const dadd_plan_refresh_desc* table,
                                     int n_desc, int n_wgs, void* stream) {
  DADD_REQUIRE(src && table, "plan_refresh: null pointer");
  DADD_REQUIRE(src_numel > 0 && n_desc > 0 && n_wgs > 0, "plan_refresh: src_numel=%lld, n_desc=%d and n_wgs=%d must be "
               "positive", src_numel, n_desc, n_wgs);
  DADD_REQUIRE(dadd_aligned16(src) && (((uintptr_t)table) & 7) == 0,
               "plan_refresh: src must be 16-byte aligned, the table 8-byte");
  dadd_launch({DADD_KNAME("plan_refresh_kernel"), 0.0, 0.0}, plan_refresh_kernel, dim3((unsigned)n_wgs), dim3(256), 0,
              static_cast<hipStream_t>(stream), static_cast<const float*>(src), src_numel, table, n_desc);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}
