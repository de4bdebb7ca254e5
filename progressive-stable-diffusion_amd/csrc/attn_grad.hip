// Backward of attention on gfx950 MFMA: gradients of O = softmax(Q K^T / sqrt(d)) V with respect to Q, K and V
// (include/dadd_hip_attn_grad.h).  Two-sided flash backward in three launches, no atomics, fp32 accumulation:
//
//  * attn_grad_stats_kernel : 64 queries per workgroup, one pass over the 64-key tiles.  Per query row the online-softmax
//                             recurrence over S^T = K Qs^T and dP^T = V dO^T (two MFMA products per tile, no PV product)
//                             gives LSE_i = m_i + log2(l_i) (log2 units) and D_i = sum_j P_ij dP_ij -> ws [B][H][Nq][2].
//                             The forward saves nothing and its output is not needed: D comes from dO . V, not dO . O.
//  * attn_grad_dkv_kernel   : one workgroup per (sample, head, 64-key tile), a wave owns 16 keys whose K and V fragments
//                             stay in registers; loop over 64-query tiles in LDS: S = Qs K^T and dP = dO V^T come out with
//                             the key on the lanes, so P and dS are already shaped as the B operand of dV^T += dO^T P and
//                             dK^T += Q^T dS (dO and Q are read transposed from their row-major LDS tiles).
//  * attn_grad_dq_kernel    : one workgroup per (sample, head, 64-query tile), a wave owns 16 queries; loop over 64-key
//                             tiles in LDS: S^T and dP^T with the query on the lanes (as flash_kernel computes its scores),
//                             dQ^T += K^T dS^T with K read transposed.
//
// The layouts are those of csrc/attention.hip: a 16x16x32 MFMA whose accumulator (rows 4g + r, column li) is repacked
// pairwise into the B operand of the next product, the contraction index permuted the same way on both operands (slot
// (g, j) of a 32-row step is row 4g + j of the first 16-row fragment for j < 4, row 4g + j - 4 of the second otherwise),
// and ds_read_b64_tr_b16 for the transposed A operand.  MFMA and VALU do not overlap on this SIMD
// (profiles/r03_y_mfma_valu_coissue.txt): there is no software pipeline here, a tile is loaded, then computed.
//
// Rounding points (the contract, restated in tests/attn_grad_reference.py):
//   Qs = q * (log2 e / sqrt(d)) in fp32, rounded to the storage type (as the forward): S = Qs . k in log2 units;
//   P  = exp2(S - LSE) in fp32; rounded to the storage type as the operand of dV = P^T dO;
//   dS = P (fp32) * (do_scale * dP - D) in fp32, rounded to the storage type as the operand of dS^T Q and dS K;
//   LSE, D, do_scale * (*do_scale_dev) and every accumulator are fp32; dV is scaled by do_scale and dK, dQ by 1/sqrt(d)
//   in fp32 and rounded once when stored.
// Masking: keys past Nk have P = 0 exactly (a select, not an underflow) and are never stored; query rows past Nq have
// P = 0 in the dkv kernel and are never stored by the dq kernel; the running maximum starts at a large finite negative
// and the first tile's rescale factor is exp2(-1e30 - m) = 0 against sums that are still 0: no inf, no 0 * inf.
//
//
// Nk is any positive count (Nq stays a multiple of 16).  Every place a key index is formed, and why no multiple of 16 is
// needed there:
//  * ag_load_tile (stats, dq): a row is read only when row < Nk - 64 kt, 16 bytes at columns 8 ch .. 8 ch + 7 < DR of
//    the head, inside the row; every other LDS row is written with zeros on every tile.  Rows past Nk are never
//    touched in memory, so they may hold anything (NaN guard rows in the tests).
//  * stats: a key past Nk gets S = AG_MASKED by a select on its index 64 kt + 16 kf + 4 g + r and then P = 0 by a select
//    on that constant; its dP = V dO^T is an exact 0 from the zero V row, so fmaf(0, 0, dacc) adds nothing.  nkt =
//    ceil(Nk / 64), so the last tile holds at least key 64 (nkt - 1): with exactly one key there, it is row 0 of the
//    tile, held by the lanes g = 0, r = 0 of fragment kf = 0; dadd_max_x16x32 unites the four g of a query column, so
//    every lane's tmax is that key's finite score and mn is finite.  l >= 1 after the tile that holds the maximum.
//  * dkv: a lane owns key krow = 64 kb0 + 16 wave + li, per lane, not per wave: nothing is wave-uniform in Nk.  A lane
//    past Nk reads the clamped row min(krow, Nk - 1) (a real row: finite where the data is) only to keep the MFMA
//    operand defined; kvalid selects P = 0, so dS = 0 * (finite) = 0, its accumulator column li gets zeros (an MFMA
//    column depends on its own B column alone, so nothing crosses to a valid key) and the store is under kvalid.
//    ag_row_frags reads 16 bytes at columns 32 s + 8 g < DR, DR a multiple of 8: inside the row for the last valid row
//    too.
//  * dq: the select on 64 kt + 16 kf + 4 g + r < Nk gives P = 0, dS = 0 * (sc * 0 - D) = 0 against the zero K / V rows,
//    and K^T dS^T reads zero rows of K for them.
//  * ag_store_row writes 4 elements at columns 16 df + 4 g < DR of rows < Nk (dkv) or < Nq (dq) only.
// No dependency on 16 was found: the old rule was the set of shapes the tests covered.  Nq keeps it because every site
// has 16 queries or a multiple of 64 and the contract test pins the refusal.
//
// Resources per workgroup of 256 threads: LDS 2 tiles of 64 x (D + 8) halfs (18 / 26 / 26 / 42 KB for d = 40 / 80 / 96 / 160) plus
// 512 B of row statistics in the dkv kernel; the d = 160 dkv kernel holds 2 x 16 x 160 fp32 of dK / dV per wave (80
// registers) beside 40 of resident K / V fragments: no instantiation needs scratch (scripts/kernel_resources.py).
#include <math.h>

#include "dadd_common.h"
#include "../../include/dadd_hip_attn_grad.h"

namespace {

constexpr int ag_round_up(int a, int b) { return (a + b - 1) / b * b; }
constexpr float AG_MASKED = -3.0e38f;     // large finite negative, never inf
constexpr float AG_M_INIT = -1.0e30f;

template <int DR>
struct AgGeom {
  static constexpr int D = ag_round_up(DR, 32), DVP = ag_round_up(DR, 16);
  static constexpr int KS = D / 32, DF = DVP / 16, DC = DR / 8;
  static constexpr int LD = D + 8;              // halfs per LDS row: 16-byte rows, columns DR .. D-1 stay zero
  static constexpr int TILE = 64 * LD;          // halfs
  static constexpr int SMEM_Q = 2 * TILE * (int)sizeof(half_t);            // stats / dq kernels: K and V
  static constexpr int SMEM_KV = SMEM_Q + 64 * 2 * (int)sizeof(float);     // dkv kernel: Q, dO and the rows' (LSE, D)
};

struct AttnGradArgs {
  const half_t* q;
  const half_t* k;
  const half_t* v;
  const half_t* dout;
  half_t* dq;
  half_t* dk;
  half_t* dv;
  float* ws;
  const float* scale_dev;
  long long bsq, bskv, bso, bsdq, bsdkv;     // elements between samples
  int B, Nq, Nk, H, ldq, ldkv, ldo, lddq, lddkv;
  float do_scale, scale_log2, inv_sqrt_d;
};

__device__ __forceinline__ h8 ag_pack(const f4& lo, const f4& hi) {   // the rounding of P / dS to the storage type
  h8 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r[j] = (half_t)lo[j];
    r[j + 4] = (half_t)hi[j];
  }
  return r;
}

__device__ __forceinline__ h8 ag_scaled(h8 x, float s) {   // x * s in fp32, rounded to the storage type
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = (half_t)((float)x[e] * s);
  return x;
}

// do_scale * (*do_scale_dev): the factor on dout, read on the device
__device__ __forceinline__ float ag_do_scale(const AttnGradArgs& p) {
  return p.scale_dev != nullptr ? p.do_scale * *p.scale_dev : p.do_scale;
}

// 64 rows x DR columns of one head from global memory (row 0 at src, row stride ld) into a row-major LDS tile; rows from
// rows_valid on are zero-filled, so that whatever they meet in a product contributes exactly 0.
template <int DR>
__device__ __forceinline__ void ag_load_tile(half_t* dst, const half_t* src, int ld, int rows_valid, int t) {
  constexpr int DC = AgGeom<DR>::DC, LD = AgGeom<DR>::LD;
  const h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int idx = t; idx < 64 * DC; idx += 256) {
    const int row = idx / DC, ch = idx - row * DC;
    *reinterpret_cast<h8*>(dst + row * LD + ch * 8) =
        row < rows_valid ? *reinterpret_cast<const h8*>(src + (size_t)row * ld + ch * 8) : zero8;
  }
}

// the fragments of one row as an MFMA operand: lane (g, li) holds columns 32 s + 8 g .. + 7 of its row
template <int DR>
__device__ __forceinline__ void ag_row_frags(h8 (&f)[AgGeom<DR>::KS], const half_t* row, int g) {
  const h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < AgGeom<DR>::KS; ++s) {
    const int dc = 32 * s + 8 * g;
    f[s] = (dc < DR) ? *reinterpret_cast<const h8*>(row + dc) : zero8;
  }
}

// C[4g + r][li] = sum_d A[row 4g + r][d] * B[row li][d]: A rows from an LDS tile (a = tile + (16 f + li) * LD + 8 g),
// B fragments resident; SCALED: the A rows are Qs = round(q * scale)
template <int DR, bool SCALED>
__device__ __forceinline__ f4 ag_rows_dot(const half_t* a, const h8 (&b)[AgGeom<DR>::KS], float scale) {
  f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < AgGeom<DR>::KS; ++s) {
    h8 av = *reinterpret_cast<const h8*>(a + 32 * s);
    if (SCALED) av = ag_scaled(av, scale);
    acc = DADD_MFMA_16X16X32(av, b[s], acc, 0, 0, 0);
  }
  return acc;
}

// acc[df][r] (column 16 df + 4 g + r of the head, lane column li) += sum over the tile's 64 rows of tile[row][col] *
// pb[row][li], the rows in the permuted order of ag_pack; tr = tile + (4 g + (li >> 2)) * LD + 4 (li & 3)
template <int DR>
__device__ __forceinline__ void ag_tr_accum(f4 (&acc)[AgGeom<DR>::DF], const half_t* tr, const h8 (&pb)[2]) {
  constexpr int LD = AgGeom<DR>::LD;
#pragma unroll
  for (int df = 0; df < AgGeom<DR>::DF; ++df) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const half_t* base = tr + kb * 32 * LD + df * 16;
      const h8 a = dadd_tr_pair(base, base + 16 * LD);
      acc[df] = DADD_MFMA_16X16X32(a, pb[kb], acc[df], 0, 0, 0);
    }
  }
}

// rows 16 df + 4 g .. + 3 of a lane's accumulator column -> 4 consecutive elements of its output row
template <int DR>
__device__ __forceinline__ void ag_store_row(half_t* row, const f4 (&acc)[AgGeom<DR>::DF], float scale, int g) {
#pragma unroll
  for (int df = 0; df < AgGeom<DR>::DF; ++df) {
    const int dcol = df * 16 + 4 * g;
    if (dcol < DR) {
      h4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (half_t)(acc[df][r] * scale);
      *reinterpret_cast<h4*>(row + dcol) = o;
    }
  }
}

template <int DR>
__device__ __forceinline__ void ag_zero_lds(half_t* lds, int t) {
  const h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = t; i < 2 * AgGeom<DR>::TILE / 8; i += 256) *reinterpret_cast<h8*>(lds + i * 8) = zero8;
}

// ---- launch 1: LSE and D per query row ------------------------------------------------------------------------------
template <int DR>
__global__ __launch_bounds__(256) void attn_grad_stats_kernel(const AttnGradArgs p) {
  using G = AgGeom<DR>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  half_t* Ks = reinterpret_cast<half_t*>(smem);
  half_t* Vs = Ks + G::TILE;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4, li = lane & 15;
  const int nqb = (p.Nq + 63) / 64;
  const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
  const int b = bh / p.H, h = bh - b * p.H;
  ag_zero_lds<DR>(Ks, t);

  const int qrow = qb * 64 + wave * 16 + li;
  const int qrc = min(qrow, p.Nq - 1);
  h8 qf[G::KS], dof[G::KS];
  ag_row_frags<DR>(qf, p.q + b * p.bsq + (size_t)qrc * p.ldq + h * DR, g);
  ag_row_frags<DR>(dof, p.dout + b * p.bso + (size_t)qrc * p.ldo + h * DR, g);
#pragma unroll
  for (int s = 0; s < G::KS; ++s) qf[s] = ag_scaled(qf[s], p.scale_log2);

  const half_t* kbase = p.k + b * p.bskv + h * DR;
  const half_t* vbase = p.v + b * p.bskv + h * DR;
  float m = AG_M_INIT, l = 0.f, dacc = 0.f;     // l and dacc: this lane's 16 keys of every tile, united at the end
  const int nkt = (p.Nk + 63) / 64;
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();   // the zero fill / everyone finished reading tile kt - 1
    ag_load_tile<DR>(Ks, kbase + (size_t)kt * 64 * p.ldkv, p.ldkv, p.Nk - kt * 64, t);
    ag_load_tile<DR>(Vs, vbase + (size_t)kt * 64 * p.ldkv, p.ldkv, p.Nk - kt * 64, t);
    __syncthreads();
    f4 sacc[4], dp[4];     // rows = keys 16 kf + 4 g + r, column = query li
    float tmax = AG_MASKED;
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      sacc[kf] = ag_rows_dot<DR, false>(Ks + (kf * 16 + li) * G::LD + 8 * g, qf, 1.f);
      dp[kf] = ag_rows_dot<DR, false>(Vs + (kf * 16 + li) * G::LD + 8 * g, dof, 1.f);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (kt * 64 + kf * 16 + 4 * g + r >= p.Nk) sacc[kf][r] = AG_MASKED;
        tmax = fmaxf(tmax, sacc[kf][r]);
      }
    }
    tmax = dadd_max_x16x32(tmax);       // every tile holds at least one key: finite
    const float mn = fmaxf(m, tmax);
    const float alpha = __builtin_amdgcn_exp2f(m - mn);    // first tile: exp2(-1e30 - mn) = 0 against l = dacc = 0
    l *= alpha;
    dacc *= alpha;
#pragma unroll
    for (int kf = 0; kf < 4; ++kf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = sacc[kf][r] == AG_MASKED ? 0.f : __builtin_amdgcn_exp2f(sacc[kf][r] - mn);
        l += pv;
        dacc = fmaf(pv, dp[kf][r], dacc);
      }
    m = mn;
  }
  l = dadd_sum_x16x32(l);
  dacc = dadd_sum_x16x32(dacc);
  if (g == 0 && qrow < p.Nq) {
    float2 st;
    st.x = m + log2f(l);
    st.y = ag_do_scale(p) * dacc / l;
    *reinterpret_cast<float2*>(p.ws + ((size_t)bh * p.Nq + qrow) * 2) = st;
  }
}

// ---- launch 2: dK and dV of one 64-key tile ---------------------------------------------------------------------------
template <int DR>
__global__ __launch_bounds__(256) void attn_grad_dkv_kernel(const AttnGradArgs p) {
  using G = AgGeom<DR>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  half_t* Qs = reinterpret_cast<half_t*>(smem);
  half_t* Os = Qs + G::TILE;
  float2* St = reinterpret_cast<float2*>(smem + G::SMEM_Q);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4, li = lane & 15;
  const int nkb = (p.Nk + 63) / 64;
  const int bh = blockIdx.x / nkb, kb0 = blockIdx.x - bh * nkb;
  const int b = bh / p.H, h = bh - b * p.H;
  ag_zero_lds<DR>(Qs, t);

  const int krow = kb0 * 64 + wave * 16 + li;
  const bool kvalid = krow < p.Nk;
  const int krc = min(krow, p.Nk - 1);
  h8 kf[G::KS], vf[G::KS];
  ag_row_frags<DR>(kf, p.k + b * p.bskv + (size_t)krc * p.ldkv + h * DR, g);
  ag_row_frags<DR>(vf, p.v + b * p.bskv + (size_t)krc * p.ldkv + h * DR, g);
  const float sc = ag_do_scale(p);

  f4 dkacc[G::DF], dvacc[G::DF];     // rows = head columns 16 df + 4 g + r, column = key li
#pragma unroll
  for (int df = 0; df < G::DF; ++df) dkacc[df] = dvacc[df] = f4{0.f, 0.f, 0.f, 0.f};

  const half_t* qbase = p.q + b * p.bsq + h * DR;
  const half_t* obase = p.dout + b * p.bso + h * DR;
  const float* wsb = p.ws + (size_t)bh * p.Nq * 2;
  const int tr_off = (4 * g + (li >> 2)) * G::LD + 4 * (li & 3);
  const int nqt = (p.Nq + 63) / 64;
  for (int qt = 0; qt < nqt; ++qt) {
    __syncthreads();
    ag_load_tile<DR>(Qs, qbase + (size_t)qt * 64 * p.ldq, p.ldq, p.Nq - qt * 64, t);
    ag_load_tile<DR>(Os, obase + (size_t)qt * 64 * p.ldo, p.ldo, p.Nq - qt * 64, t);
    if (t < 64) St[t] = *reinterpret_cast<const float2*>(wsb + (size_t)min(qt * 64 + t, p.Nq - 1) * 2);
    __syncthreads();
    f4 pm[4], ds[4];       // rows = queries 16 f + 4 g + r, column = key li
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const f4 s = ag_rows_dot<DR, true>(Qs + (f * 16 + li) * G::LD + 8 * g, kf, p.scale_log2);
      const f4 dp = ag_rows_dot<DR, false>(Os + (f * 16 + li) * G::LD + 8 * g, vf, 1.f);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = f * 16 + 4 * g + r;
        const float2 st = St[qi];
        const float pv = (kvalid && qt * 64 + qi < p.Nq) ? __builtin_amdgcn_exp2f(s[r] - st.x) : 0.f;
        pm[f][r] = pv;
        ds[f][r] = pv * (sc * dp[r] - st.y);
      }
    }
    h8 pbp[2], pbs[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      pbp[kb] = ag_pack(pm[2 * kb], pm[2 * kb + 1]);
      pbs[kb] = ag_pack(ds[2 * kb], ds[2 * kb + 1]);
    }
    ag_tr_accum<DR>(dvacc, Os + tr_off, pbp);     // dV^T += dO^T P
    ag_tr_accum<DR>(dkacc, Qs + tr_off, pbs);     // dK^T += Q^T dS
  }
  if (kvalid) {
    const size_t off = b * p.bsdkv + (size_t)krow * p.lddkv + h * DR;
    if (p.dk != nullptr) ag_store_row<DR>(p.dk + off, dkacc, p.inv_sqrt_d, g);
    if (p.dv != nullptr) ag_store_row<DR>(p.dv + off, dvacc, sc, g);
  }
}

// ---- launch 3: dQ of one 64-query tile --------------------------------------------------------------------------------
template <int DR>
__global__ __launch_bounds__(256) void attn_grad_dq_kernel(const AttnGradArgs p) {
  using G = AgGeom<DR>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  half_t* Ks = reinterpret_cast<half_t*>(smem);
  half_t* Vs = Ks + G::TILE;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4, li = lane & 15;
  const int nqb = (p.Nq + 63) / 64;
  const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
  const int b = bh / p.H, h = bh - b * p.H;
  ag_zero_lds<DR>(Ks, t);

  const int qrow = qb * 64 + wave * 16 + li;
  const int qrc = min(qrow, p.Nq - 1);
  h8 qf[G::KS], dof[G::KS];
  ag_row_frags<DR>(qf, p.q + b * p.bsq + (size_t)qrc * p.ldq + h * DR, g);
  ag_row_frags<DR>(dof, p.dout + b * p.bso + (size_t)qrc * p.ldo + h * DR, g);
#pragma unroll
  for (int s = 0; s < G::KS; ++s) qf[s] = ag_scaled(qf[s], p.scale_log2);
  const float2 st = *reinterpret_cast<const float2*>(p.ws + ((size_t)bh * p.Nq + qrc) * 2);
  const float sc = ag_do_scale(p);

  f4 dqacc[G::DF];       // rows = head columns 16 df + 4 g + r, column = query li
#pragma unroll
  for (int df = 0; df < G::DF; ++df) dqacc[df] = f4{0.f, 0.f, 0.f, 0.f};

  const half_t* kbase = p.k + b * p.bskv + h * DR;
  const half_t* vbase = p.v + b * p.bskv + h * DR;
  const int tr_off = (4 * g + (li >> 2)) * G::LD + 4 * (li & 3);
  const int nkt = (p.Nk + 63) / 64;
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();
    ag_load_tile<DR>(Ks, kbase + (size_t)kt * 64 * p.ldkv, p.ldkv, p.Nk - kt * 64, t);
    ag_load_tile<DR>(Vs, vbase + (size_t)kt * 64 * p.ldkv, p.ldkv, p.Nk - kt * 64, t);
    __syncthreads();
    f4 ds[4];              // rows = keys 16 kf + 4 g + r, column = query li
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      const f4 s = ag_rows_dot<DR, false>(Ks + (kf * 16 + li) * G::LD + 8 * g, qf, 1.f);
      const f4 dp = ag_rows_dot<DR, false>(Vs + (kf * 16 + li) * G::LD + 8 * g, dof, 1.f);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = (kt * 64 + kf * 16 + 4 * g + r < p.Nk) ? __builtin_amdgcn_exp2f(s[r] - st.x) : 0.f;
        ds[kf][r] = pv * (sc * dp[r] - st.y);
      }
    }
    h8 pbs[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) pbs[kb] = ag_pack(ds[2 * kb], ds[2 * kb + 1]);
    ag_tr_accum<DR>(dqacc, Ks + tr_off, pbs);     // dQ^T += K^T dS^T
  }
  if (qrow < p.Nq) ag_store_row<DR>(p.dq + b * p.bsdq + (size_t)qrow * p.lddq + h * DR, dqacc, p.inv_sqrt_d, g);
}

// ---- kernel table ---------------------------------------------------------------------------------------------------
typedef void (*AgKernel)(const AttnGradArgs);
struct AgEntry {
  int d;
  AgKernel stats, dkv, dq;
  int smem_q, smem_kv;
  const char* stats_name;
  const char* dkv_name;
  const char* dq_name;
};
#define AG_ENTRY(DR)                                                                                             \
  {DR, attn_grad_stats_kernel<DR>, attn_grad_dkv_kernel<DR>, attn_grad_dq_kernel<DR>, AgGeom<DR>::SMEM_Q,        \
   AgGeom<DR>::SMEM_KV, DADD_KNAME("attn_grad_stats_kernel") "<" #DR ">", DADD_KNAME("attn_grad_dkv_kernel") "<" #DR ">", \
   DADD_KNAME("attn_grad_dq_kernel") "<" #DR ">"}
// the head dims of the UNet's attn1 / attn2 and, 96, of the conditioning front-end's nn.MultiheadAttention(768, 8)
const AgEntry AG_TABLE[] = {AG_ENTRY(40), AG_ENTRY(80), AG_ENTRY(96), AG_ENTRY(160)};
#undef AG_ENTRY

const AgEntry* ag_find(int d) {
  for (const AgEntry& e : AG_TABLE)
    if (e.d == d) return &e;
  return nullptr;
}

}  // namespace

int dadd_init_attn_grad() {
  for (const AgEntry& e : AG_TABLE) {
    DADD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(e.stats), hipFuncAttributeMaxDynamicSharedMemorySize, e.smem_q));
    DADD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(e.dkv), hipFuncAttributeMaxDynamicSharedMemorySize, e.smem_kv));
    DADD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(e.dq), hipFuncAttributeMaxDynamicSharedMemorySize, e.smem_q));
  }
  return DADD_OK;
}

#ifndef DADD_BF16
// host only, one copy for both storage types
extern "C" long long dadd_attn_grad_ws_floats(int B, int heads, int Nq) {
  if (B <= 0 || heads <= 0 || Nq <= 0) return -1;
  return (long long)B * heads * Nq * 2;
}
#endif

extern "C" int dadd_attn_grad_f16(const dadd_attn_grad_desc* d, void* stream) {
  DADD_REQUIRE(d, "attn_grad: null descriptor");
  DADD_REQUIRE(d->q && d->k && d->v && d->dout && d->ws, "attn_grad: null pointer");
  DADD_REQUIRE(d->dq || d->dk || d->dv, "attn_grad: no output");
  const AgEntry* e = ag_find(d->d);
  DADD_REQUIRE(e != nullptr, "attn_grad: unsupported head dim %d (40, 80, 96, 160)", d->d);
  DADD_REQUIRE(d->B > 0 && d->heads > 0, "attn_grad: empty problem");
  DADD_REQUIRE(d->Nq >= 16 && d->Nq % 16 == 0, "attn_grad: Nq=%d must be a multiple of 16", d->Nq);
  DADD_REQUIRE(d->Nk >= 1, "attn_grad: Nk=%d must be positive", d->Nk);
  const int C = d->heads * d->d;
  DADD_REQUIRE(d->ld_q % 8 == 0 && d->ld_kv % 8 == 0 && d->ld_do % 8 == 0 && d->ld_dq % 8 == 0 && d->ld_dkv % 8 == 0,
               "attn_grad: leading dimensions must be multiples of 8");
  DADD_REQUIRE(d->ld_q >= C && d->ld_kv >= C && d->ld_do >= C && (!d->dq || d->ld_dq >= C) &&
                   (!(d->dk || d->dv) || d->ld_dkv >= C), "attn_grad: leading dimensions below heads * d");
  DADD_REQUIRE(d->bs_q >= 0 && d->bs_kv >= 0 && d->bs_do >= 0 && d->bs_dq >= 0 && d->bs_dkv >= 0 && d->bs_q % 8 == 0 &&
                   d->bs_kv % 8 == 0 && d->bs_do % 8 == 0 && d->bs_dq % 8 == 0 && d->bs_dkv % 8 == 0,
               "attn_grad: sample strides must be non-negative multiples of 8");
  DADD_REQUIRE(dadd_aligned16(d->q) && dadd_aligned16(d->k) && dadd_aligned16(d->v) && dadd_aligned16(d->dout) &&
                   dadd_aligned16(d->dq) && dadd_aligned16(d->dk) && dadd_aligned16(d->dv),
               "attn_grad: pointers must be 16-byte aligned");
  DADD_REQUIRE((((uintptr_t)d->ws) & 7) == 0, "attn_grad: ws must be 8-byte aligned");
  const long long bh = (long long)d->B * d->heads;
  DADD_REQUIRE(bh * ((d->Nq + 63) / 64) <= 0x7fffffffLL && bh * ((d->Nk + 63) / 64) <= 0x7fffffffLL,
               "attn_grad: too many workgroups");
  AttnGradArgs a;
  a.q = static_cast<const half_t*>(d->q);
  a.k = static_cast<const half_t*>(d->k);
  a.v = static_cast<const half_t*>(d->v);
  a.dout = static_cast<const half_t*>(d->dout);
  a.dq = static_cast<half_t*>(d->dq);
  a.dk = static_cast<half_t*>(d->dk);
  a.dv = static_cast<half_t*>(d->dv);
  a.ws = d->ws;
  a.scale_dev = d->do_scale_dev;
  a.B = d->B; a.Nq = d->Nq; a.Nk = d->Nk; a.H = d->heads;
  a.ldq = d->ld_q; a.ldkv = d->ld_kv; a.ldo = d->ld_do; a.lddq = d->ld_dq; a.lddkv = d->ld_dkv;
  a.bsq = d->bs_q ? d->bs_q : (long long)d->Nq * d->ld_q;
  a.bskv = d->bs_kv ? d->bs_kv : (long long)d->Nk * d->ld_kv;
  a.bso = d->bs_do ? d->bs_do : (long long)d->Nq * d->ld_do;
  a.bsdq = d->bs_dq ? d->bs_dq : (long long)d->Nq * d->ld_dq;
  a.bsdkv = d->bs_dkv ? d->bs_dkv : (long long)d->Nk * d->ld_dkv;
  a.do_scale = d->do_scale;
  a.inv_sqrt_d = 1.0f / sqrtf((float)d->d);
  a.scale_log2 = 1.4426950408889634f / sqrtf((float)d->d);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned gq = (unsigned)(bh * ((d->Nq + 63) / 64)), gk = (unsigned)(bh * ((d->Nk + 63) / 64));
  const double pairs = (double)bh * d->Nq * d->Nk * d->d;       // multiply-adds of one Nq x Nk x d product
  const double qbytes = (double)bh * d->Nq * d->d * 2.0, kbytes = (double)bh * d->Nk * d->d * 2.0;
  dadd_launch({e->stats_name, 4.0 * pairs, 2.0 * qbytes + 2.0 * kbytes}, e->stats, dim3(gq), dim3(256), (unsigned)e->smem_q, s, a);
  DADD_LAUNCH_CHECK();
  if (d->dk || d->dv) {
    dadd_launch({e->dkv_name, 8.0 * pairs, 2.0 * qbytes + 4.0 * kbytes}, e->dkv, dim3(gk), dim3(256), (unsigned)e->smem_kv, s, a);
    DADD_LAUNCH_CHECK();
  }
  if (d->dq) {
    dadd_launch({e->dq_name, 6.0 * pairs, 3.0 * qbytes + 2.0 * kbytes}, e->dq, dim3(gq), dim3(256), (unsigned)e->smem_q, s, a);
    DADD_LAUNCH_CHECK();
  }
  return DADD_OK;
}
