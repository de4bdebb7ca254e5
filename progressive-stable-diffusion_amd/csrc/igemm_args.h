// Kernel argument block shared by the two implicit-GEMM kernels (igemm.hip, igemm_dma.hip).
#pragma once
#include "dadd_common.h"
#include "fastdiv.h"

struct IgemmArgs {
  const half_t* x;
  const half_t* x2;
  const half_t* w;
  half_t* out;
  float* partial;
  const float* bias;
  const float* rowvec;
  const half_t* residual;
  int* counters;   // split-K tickets, one per output tile, zero between launches (nullptr: finish kernel)
  float* gn_ws;         // DADD_EPI_GNSTAT: GroupNorm chunk partials [B][gn_nchunk][32][2] written by the epilogue
  int gn_nchunk, gn_cg;  //   chunks per sample (= Ho*Wo / rows per MFMA wave), channels per group
  const float* ln_c1;   // DADD_EPI_LNFOLD: c1[n] = sum_k w[n][k] (w already carries the LayerNorm gamma)
  float ln_eps;
  float* ln_stats_out;        // DADD_EPI_LNSTAT: row partials of the OUTPUT, [N / WN][M][2] (WN = columns per MFMA wave)
  const float* ln_stats_in;   // DADD_EPI_LNFOLD with the statistics of x supplied by its producer: [ln_parts_in][M][2]
  int ln_parts_in;
  const float* gni_ws;        // DADD_PRE_GN: chunk partials of the input [B][gni_nchunk][32][2], affine, eps
  const float* gni_gamma;
  const float* gni_beta;
  int gni_nchunk;
  float gni_eps;
  const float* gni_ws2;       // ... of the second source (skip-concat): its own 32 groups over C2 channels
  int gni_nchunk2;
  half_t* gno_out;            // DADD_EPI_GNAPPLY: GroupNorm (+ SiLU) of the OUTPUT written beside it by the split-K finish
  const float* gno_gamma;
  const float* gno_beta;
  float gno_eps;
  int B, Hi, Wi, C1, C2, Ho, Wo, N;
  int taps, stride, ups, pad;   // ups: 0, 1 (9-tap gather on the virtual 2Hi x 2Wi image) or 2 (four phase convs, w = the folded weights)
  int ldo, ldr, ld_rowvec;
  int splitk, flags;
  int M, K, nkt, kps, ntiles;
  int korder;           // LDS-DMA kernel only: 0 = channels fastest, 1 = taps fastest (3x3)
  int mtiles, gm, gn;   // tile order: groups of gm x gn tiles (one of them spans its whole dimension); gm == 0: n fastest
  // Division-free prologue (fastdiv.h), filled by dadd_igemm_resolve.  fd_on: M, K and the tile count are below 2^24, so
  // every dividend of the kernels is in range; otherwise the kernels divide.  plain: a linear layer (one tap, stride 1,
  // no padding, output map == input map) — output row m reads input pixel m, no decode at all.
  int fd_on, plain;
  dadd_fastdiv fd_howo, fd_wo, fd_cin;   // row -> (sample, y, x); K offset -> tap
  dadd_fastdiv fd_t0, fd_t1, fd_t2;      // tile_decode: tiles per group (or ntiles), row tiles per group, column groups
  int ngn;                               // ntiles / gn (2-D groups)
  int pf_kt;                             // run-ahead weight prefetch (below): K tiles of a slice that are prefetched, 0 = none
};

// ---- run-ahead prefetch of the weight strip (igemm_dma.hip) -------------------------------------------------------
// The weights are cold at every launch of a step.  All p.mtiles row-tile workgroups of one column
// tile and K slice stream the SAME weight strip, each through a ring with three K tiles in flight, so the whole chip has
// only those three tiles of a strip on their way from HBM.  The MFMA waves, idle until the first K tiles have landed,
// therefore touch the first pf_kt K tiles of the strip ahead of the rings — one dword per 128-byte line, the lines
// dealt round-robin over the sharing workgroups (workgroup mt takes lines mt, mt + mtiles, ...), so every line is
// requested once and a workgroup issues a handful of loads.  (Every workgroup touching its WHOLE strip was measured
// first and is slower than no prefetch, hot and cold: 2,000 single-line requests per workgroup queue in the CU's one
// vector-memory pipe ahead of the ring DMA, profiles/r11_*.  The halo conv and strips shared by only eight workgroups
// measured no gain in the shared form and have none.)  The descriptor has the base and num_records of the DMA's;
// rows past N and lines past the slice get an out-of-range offset and move nothing.  The loads are never consumed.
// They all name ONE destination register that the caller keeps alive until dadd_pf_drain — an s_waitcnt vmcnt(0) in
// front of the epilogue, where they are long complete — because the compiler does not know that a load is outstanding
// on an inline-asm result and would hand the register to the main loop otherwise.  Only the MFMA waves may issue them:
// the loader waves' counted vmcnt waits assume that nothing but their ring DMA is in flight.
// DADD_PF_KTILES: how far ahead, in K tiles of a launch slice (0 = no prefetch); DADD_PF_MIN_SHARE: fewest workgroups
// per strip for which dadd_igemm_resolve turns it on.  The macros exist for the sweep builds; the product library is
// built without them.
#ifndef DADD_PF_KTILES
#define DADD_PF_KTILES 24
#endif
#ifndef DADD_PF_MIN_SHARE
#define DADD_PF_MIN_SHARE 16
#endif
typedef unsigned dadd_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ dadd_u4 dadd_pf_desc(const void* base, int bytes) {
  const unsigned long long a = (unsigned long long)base;
  return dadd_u4{(unsigned)a, (unsigned)(a >> 32) & 0xFFFFu, (unsigned)bytes, 0x00020000u};
}
__device__ __forceinline__ void dadd_pf_line(unsigned& sink, unsigned off, dadd_u4 desc) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "+v"(sink) : "v"(off), "s"(desc));
#endif
}
__device__ __forceinline__ void dadd_pf_drain(unsigned& sink) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(sink)::"memory");
#endif
}

// output row -> sample (rowvec / GroupNorm-statistics addressing) and -> (sample, y, x) (the im2col gather)
__device__ __forceinline__ int row_sample(const IgemmArgs& p, int m, int HoWo) {
  return p.fd_on ? (int)dadd_fastdiv_div((uint32_t)m, p.fd_howo) : m / HoWo;
}
__device__ __forceinline__ void row_decode(const IgemmArgs& p, int m, int HoWo, int& b, int& oy, int& ox) {
  b = row_sample(p, m, HoWo);
  const int rem = m - b * HoWo;
  oy = p.fd_on ? (int)dadd_fastdiv_div((uint32_t)rem, p.fd_wo) : rem / p.Wo;
  ox = rem - oy * p.Wo;
}

// DADD_TUNE_UPS_FOLD (igemm_ups_fold.hip; igemm_dma_kernel.h UPS = 2): row r of a phase -> input pixel (sample, y, x).  In that mode fd_howo and
// fd_wo divide by Hi*Wi and Wi.
__device__ __forceinline__ void ups_fold_decode(const IgemmArgs& p, int r, int& b, int& y, int& x) {
  const int HiWi = p.Hi * p.Wi;
  b = p.fd_on ? (int)dadd_fastdiv_div((uint32_t)r, p.fd_howo) : r / HiWi;
  const int rem = r - b * HiWi;
  y = p.fd_on ? (int)dadd_fastdiv_div((uint32_t)rem, p.fd_wo) : rem / p.Wi;
  x = rem - y * p.Wi;
}

// XCD-aware tile order.  Workgroups are dealt round-robin over the 8 XCDs (id % 8 shares an XCD, each
// with a private 4 MiB L2).  Remap so that one XCD owns a CONTIGUOUS range of logical tiles: row
// tiles that share halo rows and all column tiles of one row tile then hit the same L2, and the nine
// taps of a 3x3 window re-read the same ~1/8 of the activation from L2 instead of from the Infinity
// Cache.  Bijective for any grid size (cdna_hip_programming.md §5 "XCD swizzle must be bijective");
// placement only affects speed, never results.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, slot = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}

// Logical tile id -> (mt, nt).  An XCD owns a contiguous range of ids (xcd_remap), so the order of ids
// decides what each 4 MiB L2 sees.  Measured with FETCH_SIZE (profiles/r01_q_traffic.txt): with n fastest
// the ntiles column tiles of one row tile start together and each of them pulls the SAME activation
// lines through the fabric (GEGLU N=2560: 198 MB fetched for 12 MB of operands), and a weight matrix
// larger than the activation is re-read by all 8 XCDs.  So: the larger operand is the one split across
// XCDs (gm < mtiles: row tiles split, A-heavy;  gn < ntiles: column tiles split, W-heavy) and inside a
// group the row tile runs fastest, so concurrent workgroups read different activation rows and share
// one or two weight tiles.  Bijective for any sizes.
__device__ __forceinline__ void tile_decode(const IgemmArgs& p, int tile_id, int& mt, int& nt) {
  if (p.gm == 0) {
    nt = tile_id % p.ntiles;
    mt = tile_id / p.ntiles;
  } else if (p.gn >= p.ntiles) {          // groups of gm row tiles x all column tiles
    const int per = p.gm * p.ntiles;
    const int g = tile_id / per, idx = tile_id - g * per;
    const int base = g * p.gm;
    const int gsz = min(p.gm, p.mtiles - base);
    mt = base + idx % gsz;
    nt = idx / gsz;
  } else if (p.gm >= p.mtiles) {          // groups of all row tiles x gn column tiles
    const int per = p.mtiles * p.gn;
    const int g = tile_id / per, idx = tile_id - g * per;
    mt = idx % p.mtiles;
    nt = g * p.gn + idx / p.mtiles;
  } else {                                // 2-D groups of gm x gn tiles (the host guarantees gm | mtiles and gn | ntiles): an XCD
    const int per = p.gm * p.gn;          // owns a block of A rows that STAYS in its L2 while the block's weight tiles stream by
    const int g = tile_id / per, idx = tile_id - g * per;
    const int ngn = p.ntiles / p.gn;
    const int gmi = g / ngn, gni = g - gmi * ngn;
    mt = gmi * p.gm + idx % p.gm;
    nt = gni * p.gn + idx / p.gm;
  }
}

// The same map with the quotients taken by multiply and shift (fd_t0 / fd_t1 / fd_t2, filled by dadd_igemm_resolve): for
// a wave-uniform id that is s_mul_hi_u32 + s_lshr_b32 on the scalar unit instead of a VALU division sequence per
// quotient.  Used by igemm_dma.hip and igemm.hip.  The halo conv keeps tile_decode: two wave-uniform quotients per launch
// and no per-lane decode — nothing was gained there (profiles/r07_b_step_profile_abc.txt).
__device__ __forceinline__ void tile_decode_fast(const IgemmArgs& p, int tile_id, int& mt, int& nt) {
  const auto div = [&](int n, const dadd_fastdiv& f, int d) { return p.fd_on ? (int)dadd_fastdiv_div((uint32_t)n, f) : n / d; };
  if (p.gm == 0) {
    mt = div(tile_id, p.fd_t0, p.ntiles);
    nt = tile_id - mt * p.ntiles;
  } else if (p.gn >= p.ntiles) {          // groups of gm row tiles x all column tiles
    const int per = p.gm * p.ntiles;
    const int g = div(tile_id, p.fd_t0, per), idx = tile_id - g * per;
    const int base = g * p.gm;
    const int gsz = min(p.gm, p.mtiles - base);
    nt = gsz == p.gm ? div(idx, p.fd_t1, p.gm) : idx / gsz;      // (the last group may be short)
    mt = base + idx - nt * gsz;
  } else if (p.gm >= p.mtiles) {          // groups of all row tiles x gn column tiles
    const int per = p.mtiles * p.gn;
    const int g = div(tile_id, p.fd_t0, per), idx = tile_id - g * per;
    const int q = div(idx, p.fd_t1, p.mtiles);
    mt = idx - q * p.mtiles;
    nt = g * p.gn + q;
  } else {                                // 2-D groups of gm x gn tiles (the host guarantees gm | mtiles and gn | ntiles): an XCD
    const int per = p.gm * p.gn;          // owns a block of A rows that STAYS in its L2 while the block's weight tiles stream by
    const int g = div(tile_id, p.fd_t0, per), idx = tile_id - g * per;
    const int gmi = div(g, p.fd_t2, p.ngn), gni = g - gmi * p.ngn;
    const int q = div(idx, p.fd_t1, p.gm);
    mt = gmi * p.gm + idx - q * p.gm;
    nt = gni * p.gn + q;
  }
}

// work of one implicit-GEMM launch as executed (roofline columns of the profiling records): the folded upsample conv
// (a.ups == 2) counts its K = 4 Cin, the MFMAs it runs, not the 9 taps of the conv it replaces
static inline double dadd_igemm_flop(const IgemmArgs& a) { return 2.0 * (double)a.M * (double)a.N * (double)a.K; }
static inline double dadd_igemm_bytes(const IgemmArgs& a) {
  const double n_out = (a.flags & DADD_EPI_GEGLU) ? a.N / 2 : a.N;
  return 2.0 * ((double)a.B * a.Hi * a.Wi * (a.C1 + a.C2) + (double)a.N * a.K * (a.ups == 2 ? 4.0 : 1.0) + (double)a.M * n_out +
                ((a.flags & DADD_EPI_RESIDUAL) ? (double)a.M * a.N : 0.0));
}

// ---- LayerNorm folded into the consuming linear (DADD_EPI_LNFOLD) -----------------------------------------------
//   LN(x) W^T + b = rstd_m * (x (gamma o W)^T - mu_m * c1) + (W beta + b),   c1[n] = sum_k gamma_k W[n][k]
// The caller passes gamma o W as the weight, c1 and the composed bias; the kernel needs mu_m and rstd_m of every
// row of its tile.  K = C for these linears, so the MFMA waves see whole rows pass through their A fragments: each
// lane accumulates sum x and sum x^2 of the 8-element pieces it reads anyway (v_dot2_f32_f16: exact products, fp32
// sums), and two xor-shuffles over the four k-quarters of a fragment finish the row — whose outputs that same lane
// owns in the swapped-MFMA layout.  No statistics pass, no normalised copy of the activation, no extra launch.
typedef half_t dadd_h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void ln_acc_pair(const h8& x, int p, float& s1, float& s2) {
  const dadd_h2 v = {x[2 * p], x[2 * p + 1]};
  const dadd_h2 one = {(half_t)1.0f, (half_t)1.0f};
  s1 = dadd_fdot2(v, one, s1);
  s2 = dadd_fdot2(v, v, s2);
}
template <int MI>
__device__ __forceinline__ void ln_finish(float (&s1)[MI], float (&s2)[MI], int K, float eps) {   // -> mu, rstd
  const float inv = 1.0f / (float)K;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    float a = s1[i], q = s2[i];
    a = dadd_sum_x16x32(a);
    q = dadd_sum_x16x32(q);
    const float mu = a * inv;
    const float var = fmaxf(q * inv - mu * mu, 0.f);
    s1[i] = mu;
    s2[i] = rsqrtf(var + eps);
  }
}

// ---- kernel table, resolve, launch ------------------------------------------------------------------------------
// Every kernel instantiation of igemm.hip, igemm_dma.hip, igemm_ups_fold.hip and conv_halo.hip is ONE row of its file's table: the name
// the profiler shows, the kernel, threads per block, dynamic LDS bytes, and the template arguments it was made from
// (`targ`, the lookup key).  The row macros build the name from the same arguments as the template-id.  dadd_init_*
// loops over a table for the LDS attribute; dadd_igemm_resolve (igemm.hip) picks rows; nothing else names a kernel.
template <typename... A>
struct KernelRow {
  const char* name;
  void (*fn)(A...);
  int threads, smem;
  int targ[5];
};
typedef KernelRow<IgemmArgs> IgemmKernel;         // the GEMM / conv kernels: void(const IgemmArgs)
typedef KernelRow<IgemmArgs, int> IgemmFinish;    // the split-K finish kernels: void(const IgemmArgs, int nsplit)

template <typename Row, int N>
inline const Row* dadd_find_row(const Row (&rows)[N], int k0, int k1 = 0, int k2 = 0, int k3 = 0, int k4 = 0) {
  for (const Row& r : rows)
    if (r.targ[0] == k0 && r.targ[1] == k1 && r.targ[2] == k2 && r.targ[3] == k3 && r.targ[4] == k4) return &r;
  return nullptr;
}
template <typename Row, int N>
inline int dadd_set_max_lds(const Row (&rows)[N]) {
  for (const Row& r : rows)
    DADD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(r.fn), hipFuncAttributeMaxDynamicSharedMemorySize, r.smem));
  return DADD_OK;
}

// What one dadd_conv_igemm_f16 call launches, decided by dadd_igemm_resolve without touching the device.
struct IgemmLaunch {
  IgemmArgs a;
  const IgemmKernel* main;
  dim3 grid;
  const IgemmFinish* finish;   // nullptr: no finish launch (one K slice, or the slabs are combined by tickets)
  dim3 fgrid;
  unsigned fsmem;
  int nsplit;                  // K slices of the main launch (grid.y)
  int tile_m, tile_n;
  bool persistent;
};
int dadd_igemm_resolve(const dadd_igemm_desc* d, int num_cu, IgemmLaunch* out);

int dadd_init_igemm_dma();
const IgemmKernel* dadd_igemm_dma_row(int tile_m, int tile_n, bool ups, bool persistent, int lnk);
int dadd_init_igemm_ups_fold();
const IgemmKernel* dadd_igemm_ups_fold_row(int tile_m, int tile_n);
int dadd_init_conv_halo();
bool dadd_conv_halo_applicable(const IgemmArgs& a, int tile_n);
int dadd_conv_halo_gn_channels(int Wo);
const IgemmKernel* dadd_conv_halo_row(int Wo, bool duo, bool gn_in);
