// Data gradient of the two resampling 3x3 convolutions (stride 2; nearest 2x upsample then conv) on gfx950 MFMA: one
// gather-GEMM for both.  include/dadd_hip_dgrad.h has the algebra; both modes are one shape of computation:
//
//   dx[b][jy*so + py][jx*so + px][c] = sum_{t < ntaps(class)} sum_n dy[b][jy*sd + ey_t][jx*sd + ex_t][n] * wt[c][slab_t][n]
//
// with (so, sd) = (2, 1) and four parity classes (py, px) of 1 / 2 / 2 / 4 taps for stride 2, and (so, sd) = (1, 2) and
// one class of 16 taps on the pre-summed weights for the upsample.  No product is spent on a zero of a dilated dy.
//
//  * workgroup = 4 waves, output tile 64 pixels of ONE class x 64 channels c; grid = (sum over classes of
//    ceil(pixels / 64), C / 64); the tile -> class map is the prefix table of at most 4 entries in the argument block,
//    filled by dadd_conv_dgrad_resolve, which the launcher and the CPU tests both call
//  * both operands are K-contiguous in memory (dy rows: N; wt rows: the class's slabs, adjacent), so both LDS tiles are
//    [64 rows][128 k] filled with coalesced 16-byte pieces and both fragments are plain ds_read_b128: lane (g, li) reads
//    k = 8g .. 8g+7 of row li.  The product is computed TRANSPOSED, D^T = wt . dy^T (A = weight rows, B = pixel rows), so
//    that an accumulator holds 4 consecutive c of one pixel; the weight rows are placed in LDS so that the two
//    accumulators (i = 0, 1) of a lane are c = 8g + 4i + r: LDS row 16i + 4a + b of a 32-row block holds c = 8a + 4i + b.
//    Each lane then stores 8 consecutive c of a pixel with one 16-byte store through ld_dx.
//  * K runs tap by tap, 128 at a time: per row of the tile (b, jy, jx) is decoded ONCE into a source offset and a mask
//    of valid taps; per tap only a scalar offset and the mask bit change, per K stage only +128.  MFMA and VALU do not
//    overlap on a gfx950 SIMD, so the index work stays out of the K loop.  The 32-k MFMA steps of a stage that lie
//    wholly past N (N = 320: the last 64 of the third stage of a tap) are skipped, a block-uniform trip count.
//  * "pad, don't mask": a source pixel outside the map, a row past the class's last pixel and the ragged K tail
//    (N % 32 != 0, N % 8 == 0: a 16-byte piece is wholly inside or outside) are ZERO pieces in LDS - of BOTH tiles for
//    the K tail, so that no stale or foreign weight meets a zero - never masked lanes.  The loads themselves are
//    unconditional, from an address inside the tensors; the zero is selected when the registers go to LDS (gload)
//  * register-staged global -> LDS, TWO stages of loads in flight (two register sets, the stage loop unrolled by two):
//    the loads of stage s + 2 are issued right after stage s went to LDS and fly under the MFMAs of stages s and s + 1.
//    The launches of the 8 x 8 and 16 x 16 maps have fewer workgroups than two per CU, each with a K of 16 x 1280, and
//    a lone workgroup hides a load only behind its own MFMAs.  Measured at 1280 @ 8 -> 16 (160 workgroups): one 64-k
//    stage in flight under lane-conditional loads 197 us, this form 149 us (profiles/r09_a_dgrad_bench.txt)
//  * the LDS row stride is 144 halfs (288 B = 72 banks).  ds_read_b128 is served in four groups of 16 lanes, group 0 =
//    lanes {0-3, 12-15} (g = 0, rows li) and {20-27} (g = 1, rows 4-11), and a 16-byte read covers 4 banks starting at
//    4 * ((18 row + g) mod 16) = 4 * ((2 row + g) mod 16): rows 0-3, 12-15 at g = 0 give {0, 2, 4, 6, 8, 10, 12, 14},
//    rows 4-11 at g = 1 give {9, 11, 13, 15, 1, 3, 5, 7} - the 16 lanes cover the 64 banks once.  The other groups are
//    the same with rows and g exchanged or g + 2; the k step (+64 B) and the fragment (+16 rows) shift all lanes alike.
//    Conflict-free.  (A 136-half stride is not: 4 * ((row + g) mod 16) puts row 12, g = 0 and row 11, g = 1 on one bank.)
//  * no atomics, no split of K: the result is the same bit pattern on every call
#include "dadd_common.h"
#include "../../include/dadd_hip_dgrad.h"

namespace {

constexpr int DG_BM = 64;           // pixels per workgroup
constexpr int DG_BC = 64;           // channels c per workgroup
constexpr int DG_BK = 128;          // k per stage
constexpr int DG_KH = DG_BK / 64;   // 64-k halves of a stage
constexpr int DG_LD = DG_BK + 16;   // LDS row stride in halfs (see above)

struct DgStage {            // one thread's share of a stage: rows r0, r0 + 32, pieces q, q + 8 of both tiles
  h8 d[2][DG_KH];
  h8 w[2][DG_KH];
  unsigned ok;              // bit 2h + i: d[i][h] counts; bit 4 + h: w[.][h] counts; the others go to LDS as zeros
};

struct DgradArgs {
  const half_t* dy;
  const half_t* wt;
  half_t* dx;
  int B, Hi, Wi, C, Ho, Wo, N;
  int so, sd;                   // step of the output pixel / of the source pixel per (jy, jx)
  int ld_dy, ld_dx, ld_wt;
  unsigned ey_bits, ex_bits;    // 2 bits per slab: source offset + 1
  int nclass, xcd_by_c;
  dadd_dgrad_class cls[DADD_DGRAD_MAX_CLASSES];
};

// slab -> (ey + 1, ex + 1), 2 bits each (header: the class order of the stride-2 slabs, 4 (e + 1) + (f + 1) for the upsample)
inline void dg_tap_bits(int mode, unsigned* ey_bits, unsigned* ex_bits) {
  unsigned by = 0, bx = 0;
  if (mode == DADD_DGRAD_STRIDE2) {
    static const int kyx[9][2] = {{1, 1}, {1, 0}, {1, 2}, {0, 1}, {2, 1}, {0, 0}, {0, 2}, {2, 0}, {2, 2}};
    for (int s = 0; s < 9; ++s) {
      by |= (unsigned)((kyx[s][0] == 0) + 1) << (2 * s);
      bx |= (unsigned)((kyx[s][1] == 0) + 1) << (2 * s);
    }
  } else {
    for (int s = 0; s < 16; ++s) {
      by |= (unsigned)(s >> 2) << (2 * s);
      bx |= (unsigned)(s & 3) << (2 * s);
    }
  }
  *ey_bits = by;
  *ex_bits = bx;
}

__global__ __launch_bounds__(256) void dgrad_kernel(const DgradArgs p) {
  __shared__ __attribute__((aligned(16))) half_t Ws[DG_BC * DG_LD];   // weight tile [c, placed as above][k]
  __shared__ __attribute__((aligned(16))) half_t Ds[DG_BM * DG_LD];   // dy tile [pixel][k] of the current tap
  __shared__ long long Out[DG_BM];                                    // element offset of the row's dx pixel, -1: no pixel

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wc = wave >> 1, wm = wave & 1;
  const int g = lane >> 4, li = lane & 15;
  // Workgroups are dealt to the 8 XCDs (one L2 each) round robin in launch order, x fastest.  With a grid_x that is a
  // multiple of 8 an XCD then owns every 8th pixel tile with ALL c tiles: dy reaches each L2 once, the weight all eight.
  // xcd_by_c (the weight is the larger operand, resolve) renumbers the workgroups so that an XCD owns a contiguous run
  // of c tiles with all their pixel tiles: the weight reaches one L2, dy all eight.  Placement only, a bijection.
  // Measured: 640 @ 32 -> 16 -10 % (49 -> 44.5 us), the 1280-channel shapes within 1 %.
  int bx = blockIdx.x, by = blockIdx.y;
  if (p.xcd_by_c) {
    const int lin = by * (int)gridDim.x + bx;
    const int swz = (lin & 7) * ((int)(gridDim.x * gridDim.y) >> 3) + (lin >> 3);
    by = swz / (int)gridDim.x;
    bx = swz - by * (int)gridDim.x;
  }
  const int c0 = by * DG_BC;

  dadd_dgrad_class k = p.cls[0];   // constant indices after unrolling: selects, no indexed copy of the argument block
#pragma unroll
  for (int i = 1; i < DADD_DGRAD_MAX_CLASSES; ++i)
    if (i < p.nclass && bx >= p.cls[i].first_tile) k = p.cls[i];
  const int Wc = (p.Wi - k.px + p.so - 1) / p.so;
  const int HcWc = ((p.Hi - k.py + p.so - 1) / p.so) * Wc;
  const int m0 = (bx - k.first_tile) * DG_BM;

  const int q = t & 7;      // 16-byte pieces q and q + 8 of a 128-k row
  const int r0 = t >> 3;    // rows r0 and r0 + 32 of both tiles
  long long src[2];         // element offset of the row's source pixel (jy * sd, jx * sd) in dy
  unsigned ok_taps[2];      // bit tap: that tap's source pixel is inside the map
  const half_t* wrow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = r0 + 32 * i;
    const int m = m0 + r;
    const bool ok = m < k.pixels;
    const int mm = ok ? m : 0;
    const int b = mm / HcWc;
    const int rem = mm - b * HcWc;
    const int jy = rem / Wc;
    const int jx = rem - jy * Wc;
    const int sy = jy * p.sd, sx = jx * p.sd;
    src[i] = (((long long)b * p.Ho + sy) * p.Wo + sx) * p.ld_dy;
    unsigned msk = 0;
    for (int tap = 0; tap < k.ntaps; ++tap) {
      const int sh = 2 * (k.first_slab + tap);
      const int y = sy + (int)((p.ey_bits >> sh) & 3) - 1, x = sx + (int)((p.ex_bits >> sh) & 3) - 1;
      msk |= (unsigned)(ok & (y >= 0) & (y < p.Ho) & (x >= 0) & (x < p.Wo)) << tap;
    }
    ok_taps[i] = msk;
    if (q == 0)
      Out[r] = ok ? (((long long)b * p.Hi + jy * p.so + k.py) * p.Wi + jx * p.so + k.px) * p.ld_dx : -1;
    const int cl = (r & 32) | (((r >> 2) & 3) << 3) | (((r >> 4) & 1) << 2) | (r & 3);   // the c that LDS row r holds
    wrow[i] = p.wt + (size_t)(c0 + cl) * p.ld_wt + (size_t)k.first_slab * p.N;
  }

  const h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  // Every load is UNCONDITIONAL, from an address that is always inside the tensors (a piece that must be zero reads the
  // first piece of its row's own source pixel / weight row instead); whether it counts is a bit of st.ok, applied when
  // the registers go to LDS.  A load under a lane condition compiles to a branch with s_waitcnt vmcnt(0) behind it: the
  // eight loads of a stage would run one after the other, each paying the full latency.  For the same reason a stage
  // past the last one (`live` false) still issues its eight loads, all of them not counting: with a load under a
  // block condition the compiler must assume that nothing was issued behind the registers it waits for, and waits for
  // the younger stage too.
  auto gload = [&](int tap, int kk, bool live, DgStage& st) {
    const int sh = 2 * ((k.first_slab + tap) & 15);      // (a stage past the end may name a 17th slab)
    const long long toff = ((long long)((int)((p.ey_bits >> sh) & 3) - 1) * p.Wo + ((int)((p.ex_bits >> sh) & 3) - 1)) * p.ld_dy;
    unsigned okb = 0;
#pragma unroll
    for (int h = 0; h < DG_KH; ++h) {
      const bool k_ok = live && kk + h * 64 + q * 8 < p.N;       // N % 8 == 0: a piece is wholly inside or outside
      const int kq = k_ok ? kk + h * 64 + q * 8 : 0;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool v = k_ok && ((ok_taps[i] >> tap) & 1);
        st.d[i][h] = *reinterpret_cast<const h8*>(p.dy + (v ? src[i] + toff + kq : src[i]));
        st.w[i][h] = *reinterpret_cast<const h8*>(wrow[i] + (k_ok ? (size_t)tap * p.N + kq : 0));
        okb |= (unsigned)v << (2 * h + i);
      }
      okb |= (unsigned)k_ok << (4 + h);
    }
    st.ok = okb;
  };

  f4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  // lane (g, li): k = 8g .. 8g+7 of row li of a 16-row fragment
  const half_t* w_rd = Ws + (wc * 32 + li) * DG_LD + g * 8;
  const half_t* d_rd = Ds + (wm * 32 + li) * DG_LD + g * 8;

  const int nstage = k.ntaps * ((p.N + DG_BK - 1) / DG_BK);
  int tap = 0, kk = 0;      // the next stage to load
  int kc = 0;               // first k (within its tap) of the stage being multiplied
  auto advance = [&]() {
    kk += DG_BK;
    if (kk >= p.N) {
      kk = 0;
      ++tap;
    }
  };
  // stage s: registers -> LDS, the loads of stage s + 2 into the freed registers, then the MFMAs of stage s
  auto step = [&](int s, DgStage& st) {
    __syncthreads();        // the previous stage's reads are done
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int h = 0; h < DG_KH; ++h) {
        *reinterpret_cast<h8*>(Ds + (r0 + 32 * i) * DG_LD + h * 64 + q * 8) = ((st.ok >> (2 * h + i)) & 1) ? st.d[i][h] : zero8;
        *reinterpret_cast<h8*>(Ws + (r0 + 32 * i) * DG_LD + h * 64 + q * 8) = ((st.ok >> (4 + h)) & 1) ? st.w[i][h] : zero8;
      }
    __syncthreads();
    gload(tap, kk, s + 2 < nstage, st);
    advance();
    const int nks = s < nstage ? min(DG_BK / 32, (p.N - kc + 31) / 32) : 0;   // block-uniform
#pragma unroll
    for (int ks = 0; ks < DG_BK / 32; ++ks) {
      if (ks < nks) {
        h8 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          a[i] = *reinterpret_cast<const h8*>(w_rd + i * 16 * DG_LD + ks * 32);
          b[i] = *reinterpret_cast<const h8*>(d_rd + i * 16 * DG_LD + ks * 32);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = DADD_MFMA_16X16X32(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    kc += DG_BK;
    if (kc >= p.N) kc = 0;
  };

  DgStage st0, st1;
  gload(tap, kk, true, st0);
  advance();
  gload(tap, kk, nstage > 1, st1);
  advance();
  for (int s = 0; s < nstage; s += 2) {   // an odd count ends with an empty step: zeros to LDS, no MFMA
    step(s, st0);
    step(s + 1, st1);
  }

  // accumulator (i, j), element r of lane (g, li): channel c = 8g + 4i + r of the wave's 32, pixel row 16j + li
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long long o = Out[wm * 32 + j * 16 + li];
    if (o >= 0) {
      h8 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = (half_t)acc[0][j][r];
        v[4 + r] = (half_t)acc[1][j][r];
      }
      *reinterpret_cast<h8*>(p.dx + o + c0 + wc * 32 + g * 8) = v;
    }
  }
}

}  // namespace

#ifndef DADD_BF16   // one host-only resolve for both 16-bit types
extern "C" int dadd_conv_dgrad_resolve(const dadd_dgrad_desc* d, dadd_dgrad_choice* out) {
  DADD_REQUIRE(d != nullptr && out != nullptr, "dgrad: null descriptor");
  DADD_REQUIRE(d->dy && d->wt && d->dx, "dgrad: null dy/wt/dx");
  DADD_REQUIRE(d->B > 0 && d->Hi > 0 && d->Wi > 0 && d->Ho > 0 && d->Wo > 0 && d->N > 0 && d->C > 0, "dgrad: non-positive shape");
  DADD_REQUIRE(d->mode == DADD_DGRAD_STRIDE2 || d->mode == DADD_DGRAD_UPS, "dgrad: mode must be DADD_DGRAD_STRIDE2 or DADD_DGRAD_UPS, got %d",
               d->mode);
  DADD_REQUIRE(d->C % 64 == 0, "dgrad: C must be a multiple of 64, got %d", d->C);
  DADD_REQUIRE(d->N % 8 == 0, "dgrad: N must be a multiple of 8, got %d", d->N);
  DADD_REQUIRE(d->Hi < (1 << 30) && d->Wi < (1 << 30), "dgrad: map too large");
  const bool ups = d->mode == DADD_DGRAD_UPS;
  if (ups)
    DADD_REQUIRE(d->Ho == 2 * d->Hi && d->Wo == 2 * d->Wi, "dgrad: Ho x Wo = %d x %d is not the 2x upsample of %d x %d", d->Ho, d->Wo,
                 d->Hi, d->Wi);
  else
    DADD_REQUIRE(d->Ho == (d->Hi - 1) / 2 + 1 && d->Wo == (d->Wi - 1) / 2 + 1,
                 "dgrad: Ho x Wo = %d x %d does not belong to a %d x %d input at stride 2", d->Ho, d->Wo, d->Hi, d->Wi);
  DADD_REQUIRE((long long)d->B * d->Ho * d->Wo < (1ll << 31) && (long long)d->B * d->Hi * d->Wi < (1ll << 31) - 4 * DG_BM,
               "dgrad: more than 2^31 pixels");
  DADD_REQUIRE(d->ld_dy % 8 == 0 && d->ld_dx % 8 == 0, "dgrad: ld_dy, ld_dx must be multiples of 8, got %d, %d", d->ld_dy, d->ld_dx);
  DADD_REQUIRE(d->ld_dy >= d->N && d->ld_dx >= d->C, "dgrad: a leading dimension is shorter than the row it strides");
  DADD_REQUIRE((long long)(ups ? 16 : 9) * d->N < (1ll << 31), "dgrad: weight row too long");
  DADD_REQUIRE(dadd_aligned16(d->dy) && dadd_aligned16(d->wt) && dadd_aligned16(d->dx), "dgrad: pointers must be 16-byte aligned");

  dadd_dgrad_choice c = {};
  int tile = 0;
  if (ups) {
    c.cls[0] = dadd_dgrad_class{0, d->B * d->Hi * d->Wi, 0, 0, 0, 16};
    c.nclass = 1;
    tile = (c.cls[0].pixels + DG_BM - 1) / DG_BM;
  } else {
    int slab = 0;
    for (int py = 0; py < 2; ++py)
      for (int px = 0; px < 2; ++px) {
        const int ntaps = (py + 1) * (px + 1);
        const int pixels = d->B * ((d->Hi - py + 1) / 2) * ((d->Wi - px + 1) / 2);
        if (pixels > 0) {     // (a 1-pixel-high or -wide map has no odd rows or columns)
          c.cls[c.nclass++] = dadd_dgrad_class{tile, pixels, py, px, slab, ntaps};
          tile += (pixels + DG_BM - 1) / DG_BM;
        }
        slab += ntaps;
      }
  }
  c.grid_x = tile;
  c.grid_y = d->C / DG_BC;
  c.block = 256;
  // which operand the XCDs divide among them (dgrad_kernel): the larger one, if the grid deals evenly to the 8 XCDs
  const long long wt_elems = (long long)d->C * (ups ? 16 : 9) * d->N, dy_elems = (long long)d->B * d->Ho * d->Wo * d->N;
  c.xcd_by_c = ((long long)c.grid_x * c.grid_y) % 8 == 0 && wt_elems > dy_elems;
  c.smem = (int)(sizeof(half_t) * (DG_BC + DG_BM) * DG_LD + sizeof(long long) * DG_BM);
  *out = c;
  return DADD_OK;
}
#endif

extern "C" int dadd_conv_dgrad_f16(const dadd_dgrad_desc* d, void* stream) {
  dadd_dgrad_choice ch;
  const int rc = dadd_conv_dgrad_resolve(d, &ch);
  if (rc != DADD_OK) return rc;
  DgradArgs a;
  a.dy = static_cast<const half_t*>(d->dy);
  a.wt = static_cast<const half_t*>(d->wt);
  a.dx = static_cast<half_t*>(d->dx);
  a.B = d->B; a.Hi = d->Hi; a.Wi = d->Wi; a.C = d->C; a.Ho = d->Ho; a.Wo = d->Wo; a.N = d->N;
  const bool ups = d->mode == DADD_DGRAD_UPS;
  a.so = ups ? 1 : 2;
  a.sd = ups ? 2 : 1;
  a.ld_dy = d->ld_dy; a.ld_dx = d->ld_dx;
  a.ld_wt = (ups ? 16 : 9) * d->N;
  dg_tap_bits(d->mode, &a.ey_bits, &a.ex_bits);
  a.nclass = ch.nclass;
  a.xcd_by_c = ch.xcd_by_c;
  double mk = 0.0;      // sum over classes of pixels * taps
  for (int i = 0; i < DADD_DGRAD_MAX_CLASSES; ++i) {
    a.cls[i] = ch.cls[i];
    mk += (double)ch.cls[i].pixels * ch.cls[i].ntaps;
  }
  const DaddLaunchTag tag = {DADD_KNAME("dgrad_kernel"), 2.0 * mk * a.N * a.C,
                             2.0 * ((double)a.B * a.Ho * a.Wo * a.N + (double)a.C * a.ld_wt + (double)a.B * a.Hi * a.Wi * a.C)};
  dadd_launch(tag, dgrad_kernel, dim3(ch.grid_x, ch.grid_y), dim3(ch.block), 0, static_cast<hipStream_t>(stream), a);
  DADD_LAUNCH_CHECK();
  return DADD_OK;
}
