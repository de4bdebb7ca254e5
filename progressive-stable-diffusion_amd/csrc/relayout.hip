// One-launch re-layout of the 16-bit weights for the data gradients (include/dadd_hip_relayout.h): reads the optimizer's
// p16, writes for every listed tensor what grad_ops.dgrad_weight / _stride2 / _ups / _cout4 produce.  HBM-bound: one read
// and one write of every weight.
//
// A workgroup of 256 lanes moves one 64 (n) x 64 (c) tile of one destination slab through 8 KiB of LDS.
//   load   lane -> (row r = tid / 8 (+32), vector v = tid % 8): one 16-byte global load of src[n0 + r][tap][c0 + 8v ..];
//          8 consecutive lanes read 128 contiguous bytes.  UPS adds up to four such loads in fp32 and rounds once.
//   LDS    row r is 64 halves = 32 dwords = one half of the 64-dword bank row; vector v goes to the 16-byte slot
//          (v + r / 8) % 8 of its row (a rotation by one slot per 8 rows).  ds_write_b128 is served in groups of 8
//          contiguous lanes: one row, 8 different slots, all 32 banks once.
//   read   lane -> (n-vector nv = tid % 8, channel pair cp = tid / 8): 8 ds_read_b32 of the dword (c0 + 2cp, c0 + 2cp + 1)
//          of rows 8nv .. 8nv + 7, i.e. dword (cp + 4nv) % 32 of each row.  ds_read_b32 is served per 32-lane half:
//          nv = 0..7 and four consecutive cp give the 32 different banks (cp + 4nv) % 32.  Without the rotation the
//          eight nv of a half would sit 8 rows = 256 dwords apart, on one bank: 8-way.
//   store  the low halves of the 8 dwords are dst[c][slab][n0 + 8nv ..], the high halves the row c + 1: two 16-byte
//          global stores; 8 consecutive lanes write 128 contiguous bytes of one destination row.
// No size needs to be a multiple of the tile: rows n >= N and vectors c >= C are neither loaded nor stored (N and C are
// multiples of 8, so a vector is whole or absent).  COUT4 (N <= 4 source rows, a few KiB) skips the LDS: one lane per
// 16-byte destination vector [c][slab][0..7] gathers its N values with 2-byte loads.
#include "dadd_common.h"
#include "../../include/dadd_hip_relayout.h"

namespace {

constexpr int RL_T = DADD_RELAYOUT_TILE;

__host__ __device__ inline int rl_src_taps(int kind, int taps) { return kind == DADD_RELAYOUT_T ? taps : 9; }
__host__ __device__ inline int rl_dst_slabs(int kind, int taps) {
  return kind == DADD_RELAYOUT_T ? taps : kind == DADD_RELAYOUT_UPS ? 16 : 9;
}
__host__ __device__ inline long long rl_dst_numel(int kind, int taps, int N, int C) {
  return kind == DADD_RELAYOUT_COUT4 ? (long long)C * 72 : (long long)C * rl_dst_slabs(kind, taps) * N;
}
__host__ __device__ inline long long rl_tiles(int kind, int taps, int N, int C) {
  if (kind == DADD_RELAYOUT_COUT4) return ((long long)C * 9 + 255) / 256;
  return (long long)rl_dst_slabs(kind, taps) * ((N + RL_T - 1) / RL_T) * ((C + RL_T - 1) / RL_T);
}

// first tap and number of taps of S(i), i = e + 1 or f + 1 (grad_ops.UPS_TAP_SETS): {2}, {1,2}, {0,1}, {0}
__device__ __forceinline__ void rl_ups_set(int i, int& k0, int& cnt) {
  k0 = i == 0 ? 2 : i == 1 ? 1 : 0;
  cnt = (i == 1 || i == 2) ? 2 : 1;
}

__device__ __forceinline__ void rl_add8(float (&acc)[8], const half_t* p) {
  const h8 a = *reinterpret_cast<const h8*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] += (float)a[e];
}

__global__ __launch_bounds__(256) void relayout_kernel(const half_t* __restrict__ src, long long src_numel,
                                                       half_t* __restrict__ dst, long long dst_numel,
                                                       const dadd_relayout_desc* __restrict__ table, int n_desc) {
  __shared__ h8 tile[RL_T * 8];
  const int tid = threadIdx.x;
  const int wg = blockIdx.x;
  int lo = 0, hi = n_desc - 1;           // the last descriptor whose tile0 is <= wg (uniform: scalar loads)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].tile0 <= wg) lo = mid; else hi = mid - 1;
  }
  const dadd_relayout_desc d = table[lo];
  const int N = d.N, C = d.C, kind = d.kind;
  int local = wg - d.tile0;
  // a table that does not fit the arrays (or a stale one) writes nothing
  if (kind < DADD_RELAYOUT_T || kind > DADD_RELAYOUT_COUT4 || N <= 0 || C <= 0 || (C & 7) || (d.taps != 1 && d.taps != 9) ||
      (kind != DADD_RELAYOUT_T && d.taps != 9) || (kind == DADD_RELAYOUT_COUT4 ? N > 4 : (N & 7) != 0) ||
      ((d.src_off | d.dst_off) & 7) || d.src_off < 0 || d.dst_off < 0 || local < 0 ||
      local >= rl_tiles(kind, d.taps, N, C) || d.src_off + (long long)N * rl_src_taps(kind, d.taps) * C > src_numel ||
      d.dst_off + rl_dst_numel(kind, d.taps, N, C) > dst_numel)
    return;
  const half_t* __restrict__ S = src + d.src_off;
  half_t* __restrict__ D = dst + d.dst_off;

  if (kind == DADD_RELAYOUT_COUT4) {
    const int idx = local * 256 + tid;   // (c, slab)
    if (idx >= C * 9) return;
    const int c = idx / 9, tap = 8 - idx % 9;
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)0.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < N) o[e] = S[((size_t)e * 9 + tap) * C + c];
    *reinterpret_cast<h8*>(D + (size_t)idx * 8) = o;
    return;
  }

  const int tn = (N + RL_T - 1) / RL_T, tc = (C + RL_T - 1) / RL_T;
  const int slab = local / (tn * tc);
  local -= slab * tn * tc;
  const int n0 = (local / tc) * RL_T, c0 = (local % tc) * RL_T;
  const size_t K = (size_t)rl_src_taps(kind, d.taps) * C;       // source row
  const size_t ld = (size_t)rl_dst_slabs(kind, d.taps) * N;     // destination row

  {
    const int v = tid & 7, c = c0 + v * 8;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int r = (tid >> 3) + 32 * pass, n = n0 + r;
      if (n < N && c < C) {
        const half_t* row = S + (size_t)n * K + c;
        h8 val;
        if (kind == DADD_RELAYOUT_UPS) {
          int ky0, nky, kx0, nkx;
          rl_ups_set(slab >> 2, ky0, nky);
          rl_ups_set(slab & 3, kx0, nkx);
          float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          rl_add8(a, row + (size_t)(3 * ky0 + kx0) * C);
          if (nky == 2) rl_add8(a, row + (size_t)(3 * ky0 + 3 + kx0) * C);
          if (nkx == 2) {
            float b[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            rl_add8(b, row + (size_t)(3 * ky0 + kx0 + 1) * C);
            if (nky == 2) rl_add8(b, row + (size_t)(3 * ky0 + 3 + kx0 + 1) * C);
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] += b[e];
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) val[e] = (half_t)a[e];
        } else {
          // S2: the tap of slab s, one hex digit each (grad_ops.STRIDE2_SLABS: 4,3,5,1,7,0,2,6,8); T: flipped
          const int tap = kind == DADD_RELAYOUT_S2 ? (int)((0x862071534ull >> (4 * slab)) & 15) : d.taps - 1 - slab;
          val = *reinterpret_cast<const h8*>(row + (size_t)tap * C);
        }
        tile[r * 8 + ((v + (r >> 3)) & 7)] = val;
      }
    }
  }
  __syncthreads();
  {
    const int nv = tid & 7, cp = tid >> 3;
    const int n = n0 + nv * 8, c = c0 + 2 * cp;
    if (n < N && c < C) {                 // C is even: row c + 1 exists with row c
      const h2* t2 = reinterpret_cast<const h2*>(tile);
      h8 ev, od;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const h2 p = t2[(nv * 8 + j) * 32 + ((cp + 4 * nv) & 31)];
        ev[j] = p[0];
        od[j] = p[1];
      }
      half_t* out = D + (size_t)c * ld + (size_t)slab * N + n;
      *reinterpret_cast<h8*>(out) = ev;
      *reinterpret_cast<h8*>(out + ld) = od;
    }
  }
}

}  // namespace

#ifndef DADD_BF16   // host-only planning: one copy in the library
extern "C" long long dadd_relayout_tiles(int kind, int taps, int N, int C) {
  if (kind < DADD_RELAYOUT_T || kind > DADD_RELAYOUT_COUT4 || N <= 0 || C <= 0 || C % 8) return -1;
  if (kind == DADD_RELAYOUT_T ? (taps != 1 && taps != 9) : taps != 9) return -1;
  if (kind == DADD_RELAYOUT_COUT4 ? N > 4 : N % 8 != 0) return -1;
  return rl_tiles(kind, taps, N, C);
}

extern "C" long long dadd_relayout_dst_numel(int kind, int taps, int N, int C) {
  if (dadd_relayout_tiles(kind, taps, N, C) < 0) return -1;
  return rl_dst_numel(kind, taps, N, C);
}

extern "C" long long dadd_dgrad_relayout_plan(dadd_relayout_desc* descs, int n, long long src_numel, long long dst_numel) {
  if (!descs || n <= 0 || src_numel <= 0 || dst_numel <= 0) {
    dadd_set_error("dgrad_relayout_plan: null table, n=%d, src_numel=%lld or dst_numel=%lld not positive", n, src_numel,
                   dst_numel);
    return -1;
  }
  long long tiles = 0, dst_end = 0;
  for (int i = 0; i < n; ++i) {
    dadd_relayout_desc& d = descs[i];
    const long long t = dadd_relayout_tiles(d.kind, d.taps, d.N, d.C);
    if (t < 0) {
      dadd_set_error("dgrad_relayout_plan: descriptor %d: kind %d, taps %d, N %d, C %d is outside the contract (N and C "
                     "multiples of 8; COUT4: N 1..4; taps 1 or 9 for T, 9 otherwise)", i, d.kind, d.taps, d.N, d.C);
      return -1;
    }
    const long long src_len = (long long)d.N * rl_src_taps(d.kind, d.taps) * d.C;
    const long long dst_len = rl_dst_numel(d.kind, d.taps, d.N, d.C);
    if (d.src_off < 0 || d.src_off % 8 || d.src_off + src_len > src_numel || d.dst_off % 8 || d.dst_off < dst_end ||
        d.dst_off + dst_len > dst_numel) {
      dadd_set_error("dgrad_relayout_plan: descriptor %d: src [%lld, +%lld) of %lld or dst [%lld, +%lld) of %lld is "
                     "misaligned (8 elements), out of range or not behind the previous destination (end %lld)", i,
                     d.src_off, src_len, src_numel, d.dst_off, dst_len, dst_numel, dst_end);
      return -1;
    }
    dst_end = d.dst_off + dst_len;
    if (tiles + t > 0x7fffffffll) {
      dadd_set_error("dgrad_relayout_plan: more than 2^31 - 1 tiles");
      return -1;
    }
    d.tile0 = (int)tiles;
    d.reserved = 0;
    tiles += t;
  }
  return tiles;
}
#endif

extern "C" int dadd_dgrad_relayout_f16(const void* src, long long src_numel, void* dst, long long dst_numel,
                                       const dadd_relayout_desc* table, int n_desc, int n_tiles, void* stream) {
  DADD_REQUIRE(src && dst && table, "dgrad_relayout: null pointer");
  DADD_REQUIRE(src_numel > 0 && dst_numel > 0 && n_desc > 0 && n_tiles > 0,
               "dgrad_relayout: src_numel=%lld, dst_numel=%lld, n_desc=%d and n_tiles=%d must be positive", src_numel,
               dst_numel, n_desc, n_tiles);
  DADD_REQUIRE(dadd_aligned16(src) && dadd_aligned16(dst) && (((uintptr_t)table) & 7) == 0,
               "dgrad_relayout: src and dst must be 16-byte aligned, the table 8-byte");
  DADD_REQUIRE(src != dst, "dgrad_relayout: src and dst must be different arrays");
  dadd_launch({DADD_KNAME("relayout_kernel"), 0.0, 0.0}, relayout_kernel, dim3((unsigned)n_tiles), dim3(256), 0,
              static_cast<hipStream_t>(stream), static_cast<const half_t*>(src), src_numel, static_cast<half_t*>(dst),
              dst_numel, table, n_desc);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}
