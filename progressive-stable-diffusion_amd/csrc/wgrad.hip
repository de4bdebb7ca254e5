// Weight gradient of Linear / conv1x1 / conv3x3 on gfx950 MFMA: a GEMM that reduces over the ROW index m = (b, oy, ox).
//
//   dW[n][tap][c] = sum_m dy[m][n] * x[gather(m, tap)][c]        db[n] = sum_m dy[m][n]
//
// Both operands are stored with the reduction index m as the slow axis (dy [M][N], x [pixels][C]), the opposite of what
// every forward GEMM here wants (K contiguous).  They are staged in LDS exactly as they come from HBM - row-major
// [64 rows of m][64 columns], coalesced 16-byte pieces - and BOTH MFMA operands are read TRANSPOSED with
// ds_read_b64_tr_b16 (the V operand of attention.hip's PV product is the precedent): lane li of a 16-lane group receives
// column li of a block of 4 rows, so a pair of reads 16 rows apart hands lane (g, li) the eight values
// m = 4g..4g+3, 16+4g..16+4g+3 of one column.  The A operand (dy^T, rows n) and the B operand (x, columns c) use the same
// permutation of the 32 m of a step, so the products pair up correctly whatever that permutation is.
//
//  * workgroup = 4 waves, output tile 64 (n) x 64 (c) of ONE tap, wave (wn, wc) owns 32 x 32 of it: 2 x 2 accumulators
//  * grid = (n tiles * splitm, taps * C / 64): slice z of the reduction covers the 32-row MFMA steps
//    [z*U/splitm, (z+1)*U/splitm) of the U = ceil(M/32), staged 64 rows at a time; rows past the slice's end are zeros
//  * ragged M, padding pixels of the 3x3 gather and ragged N are ZEROS in the LDS tile, never masked lanes: the transposed
//    read gathers across lanes and needs EXEC all ones; zero rows add nothing to the sums ("pad, don't mask")
//  * the LDS row stride is 80 halfs (160 B = 40 banks): the 8 rows x 32 B a 32-lane half touches in one transposed read
//    fall on 8 distinct groups of 8 banks (0, 40, 16, 56, 32, 8, 48, 24) - conflict-free, and every lane's address is a
//    multiple of 8 bytes (row stride 160, column offsets 32 * block + 8 * p)
//  * splitm > 1: every slice writes its own fp32 slab [N][taps][C] (+ N bias sums) into `partial`; wgrad_finish_kernel
//    adds the slabs in slice order.  No floating-point atomics: the result is the same bit pattern on every call.
//  * db: the workgroups of the first (tap, c) block column-sum the dy tile they have in LDS anyway (wave 0, one column per lane)
#include <algorithm>

#include "dadd_common.h"
#include "../../include/dadd_hip_grad.h"

namespace {

constexpr int WG_BM = 64;   // rows of m per stage
constexpr int WG_BN = 64;   // output rows (n) per workgroup
constexpr int WG_BC = 64;   // output columns (c) per workgroup
constexpr int WG_LD = 80;   // LDS row stride in halfs (see above)

struct WgradArgs {
  const half_t* dy;
  const half_t* x;
  float* dw;
  float* dbias;
  float* partial;
  int B, Hi, Wi, C, Ho, Wo, N, M;
  int taps, stride, ups, pad;
  int ld_dy, ld_x, ld_dw, ld_tap;
  int splitm, nu, nnt;    // slices, 32-row steps of m, 64-row n tiles
};

__global__ __launch_bounds__(256) void wgrad_kernel(const WgradArgs p) {
  __shared__ __attribute__((aligned(16))) half_t As[WG_BM * WG_LD];   // dy tile [m][n]
  __shared__ __attribute__((aligned(16))) half_t Bs[WG_BM * WG_LD];   // x tile  [m][c] of this block's tap

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wn = wave >> 1, wc = wave & 1;
  const int g = lane >> 4, li = lane & 15;
  const int z = blockIdx.x / p.nnt;
  const int n0 = (blockIdx.x - z * p.nnt) * WG_BN;
  const int cpt = p.C / WG_BC;
  const int tap = blockIdx.y / cpt;
  const int c0 = (blockIdx.y - tap * cpt) * WG_BC;
  const int ky = (p.taps == 9) ? tap / 3 : 0;
  const int kx = (p.taps == 9) ? tap - 3 * ky : 0;
  const int m_beg = (int)((long long)z * p.nu / p.splitm) * 32;                       // this slice's rows [m_beg, m_end)
  const int m_end = min((int)((long long)(z + 1) * p.nu / p.splitm) * 32, p.M);
  const int Hv = p.ups ? 2 * p.Hi : p.Hi;
  const int Wv = p.ups ? 2 * p.Wi : p.Wi;
  const int HoWo = p.Ho * p.Wo;
  const int q = t & 7;      // 16-byte piece of a 64-column row
  const int r0 = t >> 3;    // rows r0 and r0 + 32 of the stage
  const bool n_ok = n0 + q * 8 < p.N;   // N % 8 == 0: a piece is wholly inside or outside
  const bool do_bias = p.dbias != nullptr && blockIdx.y == 0 && wave == 0;   // wave-uniform

  const h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  auto gload = [&](int m_base, h8 (&ra)[2], h8 (&rb)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m_base + r0 + 32 * i;
      const bool ok = m < m_end;
      const int mm = ok ? m : 0;
      ra[i] = (ok && n_ok) ? *reinterpret_cast<const h8*>(p.dy + (size_t)mm * p.ld_dy + n0 + q * 8) : zero8;
      const int b = mm / HoWo;
      const int rem = mm - b * HoWo;
      const int oy = rem / p.Wo;
      const int ox = rem - oy * p.Wo;
      int iy = oy * p.stride + ky - p.pad, ix = ox * p.stride + kx - p.pad;
      const bool in = ok & (iy >= 0) & (iy < Hv) & (ix >= 0) & (ix < Wv);
      if (p.ups) {
        iy >>= 1;
        ix >>= 1;
      }
      const size_t pix = in ? ((size_t)b * p.Hi + iy) * p.Wi + ix : 0;
      rb[i] = in ? *reinterpret_cast<const h8*>(p.x + pix * p.ld_x + c0 + q * 8) : zero8;
    }
  };

  f4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;

  // lane (g, li): row 4g + (li >> 2) of a 4-row block, columns 4 (li & 3) .. + 3 of its 16 - the address the transposed
  // read wants from this lane; the data it gets back is column li of the block
  const int tr_off = (4 * g + (li >> 2)) * WG_LD + 4 * (li & 3);
  const half_t* a_rd = As + tr_off + wn * 32;
  const half_t* b_rd = Bs + tr_off + wc * 32;

  h8 ra[2], rb[2];
  gload(m_beg, ra, rb);
  for (int m_base = m_beg; m_base < m_end; m_base += WG_BM) {   // block-uniform bounds: EXEC is all ones at every transposed read
    __syncthreads();                                            // the previous stage's reads are done
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<h8*>(As + (r0 + 32 * i) * WG_LD + q * 8) = ra[i];
      *reinterpret_cast<h8*>(Bs + (r0 + 32 * i) * WG_LD + q * 8) = rb[i];
    }
    __syncthreads();
    if (m_base + WG_BM < m_end) gload(m_base + WG_BM, ra, rb);   // in flight under the MFMAs
    if (do_bias) {
#pragma unroll 8
      for (int r = 0; r < WG_BM; ++r) bsum += (float)As[r * WG_LD + lane];
    }
#pragma unroll
    for (int ks = 0; ks < WG_BM / 32; ++ks) {
      h8 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const half_t* pa = a_rd + ks * 32 * WG_LD + i * 16;
        const half_t* pb = b_rd + ks * 32 * WG_LD + i * 16;
        a[i] = dadd_tr_pair(pa, pa + 16 * WG_LD);
        b[i] = dadd_tr_pair(pb, pb + 16 * WG_LD);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = DADD_MFMA_16X16X32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }

  // accumulator element r of lane (g, li): row n = 4g + r, column c = li of the 16 x 16 fragment
  float* dst;
  size_t ldn, ldt;
  if (p.splitm > 1) {
    const size_t slab = (size_t)p.N * p.taps * p.C + p.N;
    dst = p.partial + (size_t)z * slab;
    ldn = (size_t)p.taps * p.C;
    ldt = p.C;
  } else {
    dst = p.dw;
    ldn = p.ld_dw;
    ldt = p.ld_tap;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + wn * 32 + i * 16 + 4 * g + r;
      if (n < p.N) {
#pragma unroll
        for (int j = 0; j < 2; ++j) dst[n * ldn + tap * ldt + c0 + wc * 32 + j * 16 + li] = acc[i][j][r];
      }
    }
  if (do_bias && n0 + lane < p.N) {
    float* bdst = p.splitm > 1 ? dst + (size_t)p.N * p.taps * p.C : p.dbias;
    bdst[n0 + lane] = bsum;
  }
}

// dW (and db) = the slabs added in slice order 0, 1, ..., splitm - 1: four consecutive c per thread
__global__ __launch_bounds__(256) void wgrad_finish_kernel(const WgradArgs p) {
  const size_t ntc = (size_t)p.N * p.taps * p.C;
  const size_t slab = ntc + p.N;
  const size_t nvec = ntc / 4 + (p.dbias ? p.N / 4 : 0);
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (size_t)gridDim.x * 256) {
    const size_t e = v * 4;
    f4 s = *reinterpret_cast<const f4*>(p.partial + e);
    for (int k = 1; k < p.splitm; ++k) s += *reinterpret_cast<const f4*>(p.partial + (size_t)k * slab + e);
    if (e < ntc) {
      const size_t tc = (size_t)p.taps * p.C;
      const size_t n = e / tc;
      const size_t rem = e - n * tc;
      const size_t tap = rem / p.C;
      const size_t c = rem - tap * p.C;
      *reinterpret_cast<f4*>(p.dw + n * p.ld_dw + tap * p.ld_tap + c) = s;
    } else {
      *reinterpret_cast<f4*>(p.dbias + (e - ntc)) = s;
    }
  }
}

}  // namespace

extern "C" int dadd_conv_wgrad_f16(const dadd_wgrad_desc* d, void* stream) {
  DADD_REQUIRE(d != nullptr, "wgrad: null descriptor");
  WgradArgs a;
  a.dy = static_cast<const half_t*>(d->dy);
  a.x = static_cast<const half_t*>(d->x);
  a.dw = d->dw;
  a.dbias = d->dbias;
  a.partial = d->partial;
  a.B = d->B; a.Hi = d->Hi; a.Wi = d->Wi; a.C = d->C; a.Ho = d->Ho; a.Wo = d->Wo; a.N = d->N;
  a.taps = d->taps; a.stride = d->stride; a.ups = d->ups; a.pad = d->pad;
  a.ld_dy = d->ld_dy; a.ld_x = d->ld_x; a.ld_dw = d->ld_dw; a.ld_tap = d->ld_tap;
  a.splitm = d->splitm;
  DADD_REQUIRE(a.dy && a.x && a.dw, "wgrad: null dy/x/dw");
  DADD_REQUIRE(a.B > 0 && a.Hi > 0 && a.Wi > 0 && a.Ho > 0 && a.Wo > 0 && a.N > 0 && a.C > 0, "wgrad: non-positive shape");
  DADD_REQUIRE((long long)a.B * a.Ho * a.Wo < (1ll << 31) - 64 && (long long)a.B * a.Hi * a.Wi < (1ll << 31),
               "wgrad: more than 2^31 rows");
  DADD_REQUIRE(a.C % 64 == 0, "wgrad: C must be a multiple of 64, got %d", a.C);
  DADD_REQUIRE(a.N % 8 == 0, "wgrad: N must be a multiple of 8, got %d", a.N);
  if (a.taps == 1) {
    DADD_REQUIRE(a.pad == 0 && a.stride == 1 && a.ups == 0 && a.Ho == a.Hi && a.Wo == a.Wi,
                 "wgrad: taps = 1 takes pad 0, stride 1, no upsample and Ho x Wo == Hi x Wi");
  } else {
    DADD_REQUIRE(a.taps == 9 && a.pad == 1, "wgrad: taps / pad must be 1 / 0 or 9 / 1, got %d / %d", a.taps, a.pad);
    DADD_REQUIRE((a.stride == 1 || a.stride == 2) && (a.ups == 0 || a.ups == 1) && !(a.ups && a.stride != 1),
                 "wgrad: a 3x3 takes stride 1 or 2, or ups = 1 with stride 1");
    const int hv = a.ups ? 2 * a.Hi : a.Hi, wv = a.ups ? 2 * a.Wi : a.Wi;
    DADD_REQUIRE(a.Ho == (hv - 1) / a.stride + 1 && a.Wo == (wv - 1) / a.stride + 1,
                 "wgrad: Ho x Wo = %d x %d does not belong to a %d x %d input (stride %d, ups %d)", a.Ho, a.Wo, a.Hi, a.Wi,
                 a.stride, a.ups);
  }
  DADD_REQUIRE(a.ld_dy % 8 == 0 && a.ld_x % 8 == 0 && a.ld_dw % 8 == 0 && a.ld_tap % 8 == 0,
               "wgrad: ld_dy, ld_x, ld_dw, ld_tap must be multiples of 8");
  DADD_REQUIRE(a.ld_dy >= a.N && a.ld_x >= a.C && a.ld_tap >= a.C && (long long)a.ld_dw >= (long long)(a.taps - 1) * a.ld_tap + a.C,
               "wgrad: a leading dimension is shorter than the row it strides");
  DADD_REQUIRE(dadd_aligned16(a.dy) && dadd_aligned16(a.x) && dadd_aligned16(a.dw) && dadd_aligned16(a.dbias) &&
                   dadd_aligned16(a.partial),
               "wgrad: pointers must be 16-byte aligned");
  a.M = a.B * a.Ho * a.Wo;
  a.nu = (a.M + 31) / 32;
  a.nnt = (a.N + WG_BN - 1) / WG_BN;
  DADD_REQUIRE(a.splitm >= 1 && a.splitm <= a.nu, "wgrad: splitm must be in [1, ceil(M / 32) = %d], got %d", a.nu, a.splitm);
  DADD_REQUIRE(a.splitm == 1 || a.partial != nullptr, "wgrad: splitm > 1 needs a partial buffer");
  DADD_REQUIRE((long long)a.nnt * a.splitm < (1ll << 31), "wgrad: grid too large");

  hipStream_t s = static_cast<hipStream_t>(stream);
  const double ntc = (double)a.N * a.taps * a.C;
  const double in_bytes = 2.0 * a.M * a.N + 2.0 * a.B * a.Hi * a.Wi * a.C;
  const double out_bytes = 4.0 * (ntc + (a.dbias ? a.N : 0));
  const DaddLaunchTag tag = {DADD_KNAME("wgrad_kernel"), 2.0 * a.M * ntc,
                             in_bytes + (a.splitm > 1 ? a.splitm * out_bytes : out_bytes)};
  dadd_launch(tag, wgrad_kernel, dim3(a.nnt * a.splitm, a.taps * (a.C / WG_BC)), dim3(256), 0, s, a);
  DADD_LAUNCH_CHECK();
  if (a.splitm > 1) {
    const DaddLaunchTag ftag = {DADD_KNAME("wgrad_finish_kernel"), 0.0, (a.splitm + 1) * out_bytes};
    const long long nvec = (long long)(ntc / 4) + (a.dbias ? a.N / 4 : 0);
    const int blocks = (int)std::min<long long>((nvec + 255) / 256, 4096);
    dadd_launch(ftag, wgrad_finish_kernel, dim3(blocks), dim3(256), 0, s, a);
    DADD_LAUNCH_CHECK();
  }
  return DADD_OK;
}
