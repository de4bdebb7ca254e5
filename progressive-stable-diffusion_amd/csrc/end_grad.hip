// Weight and bias gradient of the UNet's 4-channel end convolutions (conv_in: fp32 NCHW latents -> Cw channels, conv_out:
// Cw channels -> fp32 NCHW) on gfx950 MFMA, and the gradient of the row-mean squared error.  include/dadd_hip_end_grad.h
// has the algebra: both weight gradients are
//
//   G[tap][t][n] = sum_p wide[p][n] * r(thin[t][p + off(tap)])      p = (b, y, x), off(tap) = (tap / 3 - 1, tap % 3 - 1)
//
// stored as dw[n][tap][t] (IN mode, [Cw][9][8] with t >= Ct zero) or dw[t][8 - tap][n] (OUT mode, [Ct][9][Cw]): a GEMM
// that reduces over the pixel index with one side 36 columns thin and the other Cw wide.  The scheme is wgrad.hip's:
//
//  * workgroup = 4 waves, output tile 48 (j = 4 tap + t, 36 used, one more for the bias) x 64 (n); wave w owns the 16
//    columns n0 + 16 w .. + 15 of it: 3 accumulators.  Both operands are staged in LDS pixel-major, 64 pixels at a
//    time, and BOTH MFMA operands are read transposed with ds_read_b64_tr_b16, through the same permutation of the 32
//    pixels of a step (wgrad.hip explains the lane map and the conflict-free row stride of 80 halfs).
//  * the wide tile [64 p][64 n] comes from HBM in coalesced 16-byte pieces, as wgrad.hip's.
//  * the thin tile [64 p][48 j] is the im2col of the NCHW planes, built in registers: thread (p = t & 63, q = t >> 6)
//    loads the Ct channels of the taps q, q + 4 (and 8 for q = 0) of its pixel - consecutive lanes are consecutive
//    pixels of a plane, so every load is coalesced -, rounds them to the storage type as the forward kernels do, and
//    writes four halfs per tap.  Column 36 is 1 for a live pixel: its row of G is sum_p wide[p][n], the bias gradient
//    of IN mode, for the price of no extra instruction (1 * wide is exact).  Columns 37..47 stay zero.
//    OUT mode's bias gradient sum_p r(thin[t][p]) is the centre tap, which wave 0 holds anyway: summed in fp32 per
//    lane, then over the wave in a fixed butterfly (workgroups of the first n tile only).
//  * grid = (Cw / 64, splitm): slice z covers the 32-pixel MFMA steps [z U / splitm, (z + 1) U / splitm) of the
//    U = ceil(M / 32).  Pixels past the slice's end, padding pixels and channels t >= Ct are ZEROS in the LDS tiles, never
//    masked lanes and never read from memory: the transposed read needs EXEC all ones ("pad, don't mask").
//  * splitm > 1: every slice writes its own fp32 slab (dw in its final layout, then the bias sums) into `partial`;
//    end_wgrad_finish_kernel adds the slabs in slice order (eight runs of consecutive slices, then the runs in a fixed
//    tree).  No floating-point atomics: the same bits on every call.
#include <algorithm>

#include "dadd_common.h"
#include "../../include/dadd_hip_end_grad.h"

namespace {

constexpr int EG_BM = 64;   // pixels per stage
constexpr int EG_BN = 64;   // wide channels per workgroup
constexpr int EG_LD = 80;   // LDS row stride in halfs (wgrad.hip)
constexpr int EG_J = 48;    // thin columns: 9 taps * 4 channels, the ones column, padding to three 16-row fragments

struct EndWgradArgs {
  const float* thin;
  const half_t* wide;
  float* dw;
  float* dbias;
  float* partial;
  int B, H, W, Ct, Cw, M;
  int ld_wide, mode, splitm, nu;
  long long ndw, slab;    // fp32 elements of dw, and of one slab (dw + the bias sums, padded to a multiple of 4)
};

__global__ __launch_bounds__(256) void end_wgrad_kernel(const EndWgradArgs p) {
  __shared__ __attribute__((aligned(16))) half_t As[EG_BM * EG_LD];   // thin im2col tile [p][j]
  __shared__ __attribute__((aligned(16))) half_t Bs[EG_BM * EG_LD];   // wide tile [p][n]

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int n0 = blockIdx.x * EG_BN;
  const int z = blockIdx.y;
  const int m_beg = (int)((long long)z * p.nu / p.splitm) * 32;                       // this slice's pixels [m_beg, m_end)
  const int m_end = min((int)((long long)(z + 1) * p.nu / p.splitm) * 32, p.M);
  const int HW = p.H * p.W;
  const int q = t & 7;      // 16-byte piece of a 64-column row of wide
  const int r0 = t >> 3;    // rows r0 and r0 + 32 of the stage
  const int ntap = wave == 0 ? 3 : 2;                                                 // taps wave, wave + 4 (, 8)
  const bool out_bias = p.mode == DADD_END_WGRAD_OUT && p.dbias != nullptr && blockIdx.x == 0 && wave == 0;   // wave-uniform

  const h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const h4 zero4 = {0, 0, 0, 0};
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};

  // The registers of one stage in flight: two 16-byte pieces of wide, the fp32 thin values of this thread's (pixel, taps)
  // as they come from memory, and what of them is live: bit i = row r0 + 32 i of wide, bit 2 + k = tap k inside the map,
  // bit 5 = the pixel itself inside the slice.
  struct EgStage {
    h8 w[2];
    float t[3][4];
    unsigned ok;
  };

  // global -> registers.  Every load is UNCONDITIONAL, from a clamped address inside the tensors (a pixel of this slice, an
  // existing channel); the zero is selected when the registers go to LDS, on the far side of a barrier.  A load under a
  // lane condition makes hipcc wait vmcnt(0) behind it, and the 14 loads of a stage then run one after the other
  // (measured: 2.2 us per stage).  Nothing past the slice or outside the map is read.
  auto gload = [&](int m_base, EgStage& st) {
    unsigned okb = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m_base + r0 + 32 * i;
      const bool ok = m < m_end;
      st.w[i] = *reinterpret_cast<const h8*>(p.wide + (size_t)(ok ? m : m_beg) * p.ld_wide + n0 + q * 8);
      okb |= (unsigned)ok << i;
    }
    const int m = m_base + lane;
    const bool ok = m < m_end;
    const int mm = ok ? m : m_beg;
    const int b = mm / HW;
    const int rem = mm - b * HW;
    const int y = rem / p.W;
    const int x = rem - y * p.W;
    const float* plane = p.thin + (size_t)b * p.Ct * HW;
    okb |= (unsigned)ok << 5;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int c = 0; c < 4; ++c) st.t[k][c] = 0.f;
      if (k < ntap) {     // wave-uniform
        const int tap = wave + 4 * k;
        const int iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
        const bool in = ok & (iy >= 0) & (iy < p.H) & (ix >= 0) & (ix < p.W);
        const int off = in ? iy * p.W + ix : rem;
#pragma unroll
        for (int c = 0; c < 4; ++c) st.t[k][c] = plane[(size_t)(c < p.Ct ? c : 0) * HW + off];
        okb |= (unsigned)in << (2 + k);
      }
    }
    st.ok = okb;
  };

  f4 acc[3];
#pragma unroll
  for (int f = 0; f < 3; ++f) acc[f] = f4{0.f, 0.f, 0.f, 0.f};

  // columns 40..47 of the thin tile are never written again
  if (wave >= 2) *reinterpret_cast<h4*>(As + lane * EG_LD + 40 + 4 * (wave - 2)) = zero4;

  // lane (g, li): row 4g + (li >> 2) of a 4-row block, columns 4 (li & 3) .. + 3 of its 16 - the address the transposed
  // read wants from this lane; the data it gets back is column li of the block
  const int tr_off = (4 * g + (li >> 2)) * EG_LD + 4 * (li & 3);
  const half_t* a_rd = As + tr_off;
  const half_t* b_rd = Bs + tr_off + wave * 16;

  // one stage: registers -> LDS (rounding thin to the storage type, zeros where the mask says so), the loads of the stage
  // after the next into the freed registers, then the MFMAs.  All bounds are block-uniform: EXEC is all ones at every
  // transposed read.
  auto stage = [&](EgStage& st, int m_next) {
    __syncthreads();                                            // the previous stage's reads are done
#pragma unroll
    for (int i = 0; i < 2; ++i)
      *reinterpret_cast<h8*>(Bs + (r0 + 32 * i) * EG_LD + q * 8) = ((st.ok >> i) & 1) ? st.w[i] : zero8;
    h4 ra[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int c = 0; c < 4; ++c) ra[k][c] = (half_t)((((st.ok >> (2 + k)) & 1) && c < p.Ct) ? st.t[k][c] : 0.f);
    if (out_bias) {     // tap 4, the pixel itself (k = 1 of wave 0): zero for a pixel past the slice
#pragma unroll
      for (int c = 0; c < 4; ++c) bsum[c] += (float)ra[1][c];
    }
    if (wave == 1) ra[2] = h4{(half_t)(((st.ok >> 5) & 1) ? 1.f : 0.f), 0, 0, 0};   // columns 36..39: the ones column of the bias row
#pragma unroll
    for (int k = 0; k < 2; ++k) *reinterpret_cast<h4*>(As + lane * EG_LD + 4 * (wave + 4 * k)) = ra[k];
    if (wave <= 1) *reinterpret_cast<h4*>(As + lane * EG_LD + 32 + 4 * wave) = ra[2];   // tap 8 | the ones column
    __syncthreads();
    if (m_next < m_end) gload(m_next, st);
#pragma unroll
    for (int ks = 0; ks < EG_BM / 32; ++ks) {
      const half_t* pb = b_rd + ks * 32 * EG_LD;
      const h8 bw = dadd_tr_pair(pb, pb + 16 * EG_LD);
#pragma unroll
      for (int f = 0; f < 3; ++f) {
        const half_t* pa = a_rd + ks * 32 * EG_LD + f * 16;
        const h8 at = dadd_tr_pair(pa, pa + 16 * EG_LD);
        acc[f] = DADD_MFMA_16X16X32(at, bw, acc[f], 0, 0, 0);
      }
    }
  };

  // Two register sets, so that the loads of TWO stages are in flight: a stage is 8 KB of wide and six MFMAs per wave, the
  // loop is bound by the latency of its loads, not by the work.
  EgStage st0, st1;
  gload(m_beg, st0);
  if (m_beg + EG_BM < m_end) gload(m_beg + EG_BM, st1);
  for (int m_base = m_beg; m_base < m_end; m_base += 2 * EG_BM) {
    stage(st0, m_base + 2 * EG_BM);
    if (m_base + EG_BM < m_end) stage(st1, m_base + 3 * EG_BM);
  }

  // accumulator element r of lane (g, li) of fragment f: row j = 16 f + 4 g + r = 4 (4 f + g) + r, i.e. tap 4 f + g and
  // thin channel r; column n = n0 + 16 wave + li.  f = 2, g = 1, r = 0 is the bias row.
  float* dst = p.splitm > 1 ? p.partial + (size_t)z * p.slab : p.dw;
  float* bdst = p.splitm > 1 ? dst + p.ndw : p.dbias;
  const int n = n0 + wave * 16 + li;
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const int tap = 4 * f + g;
    if (tap < 9) {
      if (p.mode == DADD_END_WGRAD_IN) {
        float* o = dst + ((size_t)n * 9 + tap) * 8;
        *reinterpret_cast<f4*>(o) = acc[f];                      // channels >= Ct: sums of exact zeros
        *reinterpret_cast<f4*>(o + 4) = f4{0.f, 0.f, 0.f, 0.f};   // the pad channels of the 8 stored
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (r < p.Ct) dst[((size_t)r * 9 + (8 - tap)) * p.Cw + n] = acc[f][r];
      }
    } else if (tap == 9 && p.mode == DADD_END_WGRAD_IN && p.dbias != nullptr) {
      bdst[n] = acc[f][0];
    }
  }
  if (out_bias) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float s = wave_sum(bsum[c]);
      if (lane == 0 && c < p.Ct) bdst[c] = s;
    }
  }
}

// dw (and dbias) = the slabs added in slice order 0, 1, ..., splitm - 1: four consecutive elements of dw per thread, then
// one bias element per thread
// The output is small (23 k floats at Cw = 320) and there is one addition per slice, so a thread per output would be
// bound by the latency of a hundred dependent loads (measured: 24 us for 103 slices).  Eight lanes share an output
// instead: lane group u (lane >> 3) adds the run of slices [u R, (u + 1) R), R = ceil(splitm / 8), in slice order, and
// the eight runs are then added as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)) by a butterfly over the lane groups - a fixed
// order that depends on splitm alone.  An output is four consecutive floats of dw, or one bias sum behind them.
__global__ __launch_bounds__(256) void end_wgrad_finish_kernel(const EndWgradArgs p) {
  const long long nvec = p.ndw / 4;
  const long long nb = p.dbias ? (p.mode == DADD_END_WGRAD_IN ? p.Cw : p.Ct) : 0;
  const int lane = threadIdx.x & 63, u = lane >> 3;
  const int run = (p.splitm + 7) / 8;
  const int k0 = min(u * run, p.splitm), k1 = min(k0 + run, p.splitm);
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6, nwave = (long long)gridDim.x * 4;
  for (long long v0 = wave * 8; v0 < nvec + nb; v0 += nwave * 8) {      // wave-uniform: every lane joins the exchanges
    const long long v = v0 + (lane & 7);
    f4 s = {0.f, 0.f, 0.f, 0.f};
    if (v < nvec) {
      const float* src = p.partial + (size_t)v * 4;
#pragma unroll 4
      for (int k = k0; k < k1; ++k) s += *reinterpret_cast<const f4*>(src + (size_t)k * p.slab);
    } else if (v < nvec + nb) {
      const float* src = p.partial + p.ndw + (size_t)(v - nvec);
#pragma unroll 4
      for (int k = k0; k < k1; ++k) s[0] += src[(size_t)k * p.slab];
    }
#pragma unroll
    for (int o = 8; o < 64; o <<= 1)
#pragma unroll
      for (int c = 0; c < 4; ++c) s[c] += __shfl_xor(s[c], o, 64);
    if (u == 0) {
      if (v < nvec)
        *reinterpret_cast<f4*>(p.dw + (size_t)v * 4) = s;
      else if (v < nvec + nb)
        p.dbias[v - nvec] = s[0];
    }
  }
}

#ifndef DADD_BF16
// out = rowgrad[b] * (2 / per) * (pred - target): grid (blocks, B), four elements per thread where VEC
template <bool VEC>
// (pred and out carry no __restrict__: out may be pred itself, every thread reads an element before it writes that element)
__global__ __launch_bounds__(256) void mse_rows_grad_kernel(const float* pred, const float* __restrict__ target,
                                                            const float* __restrict__ rowgrad, float* out, int64_t per) {
  const int b = blockIdx.y;
  const float s = rowgrad[b] * (2.0f / (float)per);
  const float* pp = pred + (size_t)b * per;
  const float* tp = target + (size_t)b * per;
  float* op = out + (size_t)b * per;
  const int64_t step = (int64_t)gridDim.x * 256;
  if (VEC) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per / 4; i += step) {
      const f4 d = *reinterpret_cast<const f4*>(pp + 4 * i) - *reinterpret_cast<const f4*>(tp + 4 * i);
      *reinterpret_cast<f4*>(op + 4 * i) = s * d;
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += step) op[i] = s * (pp[i] - tp[i]);
  }
}
#endif  // !DADD_BF16

// fp32 elements of dw and of one slab of `partial`
inline void eg_sizes(int mode, int Ct, int Cw, long long* ndw, long long* slab) {
  *ndw = mode == DADD_END_WGRAD_IN ? (long long)Cw * 72 : (long long)Ct * 9 * Cw;
  *slab = *ndw + (mode == DADD_END_WGRAD_IN ? Cw : 4);
}

}  // namespace

extern "C" int dadd_conv_end_wgrad_f16(const dadd_end_wgrad_desc* d, void* stream) {
  DADD_REQUIRE(d != nullptr, "end_wgrad: null descriptor");
  EndWgradArgs a;
  a.thin = d->thin;
  a.wide = static_cast<const half_t*>(d->wide);
  a.dw = d->dw;
  a.dbias = d->dbias;
  a.partial = d->partial;
  a.B = d->B; a.H = d->H; a.W = d->W; a.Ct = d->Ct; a.Cw = d->Cw;
  a.ld_wide = d->ld_wide; a.mode = d->mode; a.splitm = d->splitm;
  DADD_REQUIRE(a.thin && a.wide && a.dw, "end_wgrad: null thin/wide/dw");
  DADD_REQUIRE(a.B > 0 && a.H > 0 && a.W > 0 && a.Cw > 0, "end_wgrad: non-positive shape");
  DADD_REQUIRE((long long)a.B * a.H * a.W < (1ll << 31) - 256, "end_wgrad: more than 2^31 - 256 pixels");
  DADD_REQUIRE(a.mode == DADD_END_WGRAD_IN || a.mode == DADD_END_WGRAD_OUT, "end_wgrad: mode must be 0 (IN) or 1 (OUT), got %d",
               a.mode);
  DADD_REQUIRE(a.Ct >= 1 && a.Ct <= 4, "end_wgrad: Ct must be in 1..4, got %d", a.Ct);
  DADD_REQUIRE(a.Cw % 64 == 0, "end_wgrad: Cw must be a multiple of 64, got %d", a.Cw);
  DADD_REQUIRE(a.ld_wide % 8 == 0 && a.ld_wide >= a.Cw, "end_wgrad: ld_wide must be a multiple of 8 and at least Cw, got %d",
               a.ld_wide);
  DADD_REQUIRE(dadd_aligned16(a.wide) && dadd_aligned16(a.dw) && dadd_aligned16(a.partial),
               "end_wgrad: wide, dw and partial must be 16-byte aligned");
  a.M = a.B * a.H * a.W;
  a.nu = (a.M + 31) / 32;
  DADD_REQUIRE(a.splitm >= 1 && a.splitm <= a.nu, "end_wgrad: splitm must be in [1, ceil(M / 32) = %d], got %d", a.nu, a.splitm);
  DADD_REQUIRE(a.splitm == 1 || a.partial != nullptr, "end_wgrad: splitm > 1 needs a partial buffer");
  DADD_REQUIRE(a.splitm <= 65535, "end_wgrad: grid too large");
  eg_sizes(a.mode, a.Ct, a.Cw, &a.ndw, &a.slab);

  hipStream_t s = static_cast<hipStream_t>(stream);
  const double in_bytes = 2.0 * a.M * a.Cw + 4.0 * a.M * a.Ct;
  const double out_bytes = 4.0 * (double)a.slab;
  const DaddLaunchTag tag = {DADD_KNAME("end_wgrad_kernel"), 2.0 * a.M * 36.0 * a.Cw,
                             in_bytes + (a.splitm > 1 ? a.splitm * out_bytes : out_bytes)};
  dadd_launch(tag, end_wgrad_kernel, dim3(a.Cw / EG_BN, a.splitm), dim3(256), 0, s, a);
  DADD_LAUNCH_CHECK();
  if (a.splitm > 1) {
    const DaddLaunchTag ftag = {DADD_KNAME("end_wgrad_finish_kernel"), 0.0, (a.splitm + 1) * out_bytes};
    const long long nthr = a.ndw / 4 + a.Cw;
    const int blocks = (int)std::min<long long>((nthr * 8 + 255) / 256, 4096);      // eight lanes per output
    dadd_launch(ftag, end_wgrad_finish_kernel, dim3(blocks), dim3(256), 0, s, a);
    DADD_LAUNCH_CHECK();
  }
  return DADD_OK;
}

#ifndef DADD_BF16
extern "C" long long dadd_end_wgrad_partial_floats(int mode, int Ct, int Cw, int splitm) {
  if ((mode != DADD_END_WGRAD_IN && mode != DADD_END_WGRAD_OUT) || Ct < 1 || Ct > 4 || Cw <= 0 || Cw % 64) return -1;
  if (splitm <= 1) return 0;
  long long ndw, slab;
  eg_sizes(mode, Ct, Cw, &ndw, &slab);
  return slab * splitm;
}

extern "C" int dadd_mse_rows_grad_f32(const float* pred, const float* target, const float* rowgrad, float* out, int B,
                                      int64_t per_sample, void* stream) {
  DADD_REQUIRE(pred && target && rowgrad && out && B > 0 && per_sample > 0, "mse_rows_grad: bad arguments");
  DADD_REQUIRE(B <= 65535, "mse_rows_grad: more than 65535 rows");
  const bool vec = per_sample % 4 == 0 && dadd_aligned16(pred) && dadd_aligned16(target) && dadd_aligned16(out);
  const int64_t nthr = vec ? per_sample / 4 : per_sample;
  const int blocks = (int)std::min<int64_t>((nthr + 255) / 256, 1024);
  const DaddLaunchTag tag = {"mse_rows_grad_kernel", 0.0, (double)B * per_sample * 12.0};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec)
    dadd_launch(tag, mse_rows_grad_kernel<true>, dim3(blocks, B), dim3(256), 0, s, pred, target, rowgrad, out, per_sample);
  else
    dadd_launch(tag, mse_rows_grad_kernel<false>, dim3(blocks, B), dim3(256), 0, s, pred, target, rowgrad, out, per_sample);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}
#endif  // !DADD_BF16
