// Epilogue shared by the two implicit-GEMM kernels: bias / time-embedding row / residual / GEGLU,
// fp16 stores of 4 consecutive channels per lane, and the split-K combine.
//
// Split-K.  Every K slice writes its fp32 slab; with `counters` the combine happens IN the launch:
// the slice that draws the last ticket of a tile re-reads all slabs in slice order (so the sum is
// bit-reproducible) and runs the epilogue.  The hand-off follows cdna_hip_programming.md §6
// Guideline 16 in its counter form: plain slab stores -> every wave s_waitcnt vmcnt(0) -> barrier ->
// one lane: agent-scope release fence, asm vmcnt(0), relaxed agent fetch_add; the last arriver does
// one agent-scope acquire, asm vmcnt(0), resets the ticket for the next launch, and a barrier
// releases the other waves to plain loads.  No spinning, no residency assumption, results do not
// depend on block placement.  Without `counters` a separate finish kernel combines the slabs.
//
// Operand loads.  The global operands of a wave's tile are bias and c1 (one quad per column block), the time-embedding
// row (one quad per column block when the wave's rows lie in one sample, else one per element) and the residual (one
// quad per element).  They are issued in batches, each kind under ONE wave-uniform flag test, and the arithmetic and
// stores of a batch follow behind a single wait.  Taken where they are used — inside the unrolled (i, j) loops, each
// under a run-time flag test — every load got an s_waitcnt vmcnt(0) of its own, which on gfx9 also waits for the
// previous store's acknowledgement: up to 3 MI J dependent round trips per tile (profiles/r12_a_epilogue_waits.txt).
// The batch is chosen per instantiation (EPI_TILE / EPI_ROWS / EPI_COLS below) by the registers it has to spare.
//   * Addresses are clamped to the last valid row and the last valid column quad, so the loads need no bounds test: a
//     lane whose element lies outside the tensor reads a valid element and never uses it.  Stores stay predicated.
//   * The arithmetic stays conditional (`flag ? v + b : v`, never `v + 0`, which would turn -0.0f into +0.0f), with
//     contraction off so that the add cannot fuse with a multiply in front of it: outputs are bit-identical to the
//     load-at-use form.
//   * Aliasing contract: `residual` may be `out` itself (same base and row pitch) and must not overlap it in any other
//     way.  Each lane reads exactly the residual elements whose outputs it later writes (the value of a clamped load is
//     never used), so reading a batch's residual ahead of its stores gives what reading every element just before its
//     own store gave.
#pragma once
#include "igemm_args.h"
#include "ln_lds.h"
#include <type_traits>

// `on ? v + b : v` with contraction off (see "Operand loads" above)
__device__ __forceinline__ f4 epi_add_if(bool on, const f4& v, const f4& b) {
#pragma clang fp contract(off)
  const f4 s = v + b;
  return on ? s : v;
}
__device__ __forceinline__ f4 epi_add_if(bool on, const f4& v, const h4& b) {
#pragma clang fp contract(off)
  const f4 s = {v[0] + (float)b[0], v[1] + (float)b[1], v[2] + (float)b[2], v[3] + (float)b[3]};
  return on ? s : v;
}
// activation of the linear itself (wave-uniform flags), before any residual
__device__ __forceinline__ void epi_activate(int flags, f4& v) {
  if (flags & DADD_EPI_QUICKGELU) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = v[r] / (1.0f + __expf(-1.702f * v[r]));
  } else if (flags & DADD_EPI_GELU) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = dadd_gelu(v[r]);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = 1.0f / (1.0f + __expf(-v[r]));
  }
}

// E[x^2] - mu^2 of the folded LayerNorm's producer partials, in a pinned form.  Written as `ex2 - mu * mu` the compiler
// was free to contract it or not, and did so per row fragment, depending on how its vectoriser had paired the
// multiplies of neighbouring rows: 64-row tiles fused every row, 128 x 128 tiles the last two of four, 128 x 160 tiles
// none (and any change to the surrounding code reshuffled that).  The variance differs in its last bit between the
// two forms, and with it every output of the row.  The table below states the form every tile has had since its
// outputs were first recorded, so that they no longer depend on the compiler's mood.
constexpr bool epi_ln_var_fused(int J, int MI, int i) { return MI == 2 || (J == 4 && i >= 2); }
__device__ __forceinline__ float epi_ln_var(bool fused, float ex2, float mu) {      // (`fused` folds after unrolling)
#pragma clang fp contract(off)
  const float mu2 = mu * mu;
  return fused ? fmaf(-mu, mu, ex2) : ex2 - mu2;
}

// How a wave batches the operand loads of its MI x J fragments ("Operand loads" above):
//   EPI_TILE  everything ahead of the first store: one wait per tile, 2 MI J + 8 J (+ 4 J with c1) registers;
//   EPI_ROWS  the column operands ahead of everything, the residual per row fragment (J quads, then that fragment's J
//             stores): MI waits, 2 J + 8 J registers.  The persistent ring, which keeps the next tile's fragments live
//             across the epilogue;
//   EPI_COLS  per column block its bias / c1 / time-embedding quads and MI residual quads, then that block's MI stores:
//             J waits, 2 MI + 12 registers.  Instantiations with no more to spare (the 768-thread halo conv has 168
//             registers per lane).
// EPI_TILE and EPI_ROWS store row fragment outer / column block inner (the 32-byte pieces of one output row leave back
// to back and combine into full lines; column-outer measured +6 us on the 128x160 qkv tile of the persistent ring).
enum { EPI_TILE = 0, EPI_ROWS = 1, EPI_COLS = 2 };

// The operands of one wave's tile (rows mw .. mw + 16 MI, columns nw .. nw + 16 J).  All indices are compile-time
// constants after unrolling, so the arrays are registers.
template <int J, int MI, int MODE>
struct EpiOperands {
  int mcl[MI], ncl[J];       // clamped row / first column of every fragment
  f4 b4[J], c4[J], r4[J];    // bias, c1, time-embedding row (of the one sample, or of the current row fragment)
  f4 rq[MI];                 // EPI_COLS, rows in several samples: the time-embedding quads of the current column block
  h4 res[J][MI];
  bool has_bias, has_rv, has_res, has_c1, rv_one;
  int b0;                    // rv_one: the sample of all the wave's rows

  __device__ __forceinline__ void init(const IgemmArgs& p, int mw, int nw, int mc, int g, int HoWo, bool with_bias,
                                       bool with_c1) {
    has_bias = with_bias && (p.flags & DADD_EPI_BIAS) != 0;
    has_c1 = with_c1;
    has_rv = (p.flags & DADD_EPI_ROWVEC) != 0;
    has_res = (p.flags & DADD_EPI_RESIDUAL) != 0;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      mcl[i] = min(mw + i * 16 + mc, p.M - 1);
      rq[i] = f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
      ncl[j] = min(nw + j * 16 + g * 4, p.N - 4);
      b4[j] = c4[j] = r4[j] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < MI; ++i) res[j][i] = h4{};
    }
    b0 = 0;
    rv_one = false;
    if (has_rv) {     // wave-uniform: first and last valid row of the wave
      b0 = row_sample(p, min(mw, p.M - 1), HoWo);
      rv_one = b0 == row_sample(p, min(mw + MI * 16 - 1, p.M - 1), HoWo);
    }
  }
  __device__ __forceinline__ void load_col(const IgemmArgs& p, int j) {      // what depends on the column block only
    if (has_c1) c4[j] = *reinterpret_cast<const f4*>(p.ln_c1 + ncl[j]);
    if (has_bias) b4[j] = *reinterpret_cast<const f4*>(p.bias + ncl[j]);
    if (rv_one) r4[j] = *reinterpret_cast<const f4*>(p.rowvec + (size_t)b0 * p.ld_rowvec + ncl[j]);
  }
  __device__ __forceinline__ void load_res(const IgemmArgs& p, int i, int j) {
    res[j][i] = *reinterpret_cast<const h4*>(p.residual + (size_t)mcl[i] * p.ldr + ncl[j]);
  }
  __device__ __forceinline__ void before(const IgemmArgs& p) {      // ahead of the loops
    if constexpr (MODE != EPI_COLS) {
      if (has_c1) {
#pragma unroll
        for (int j = 0; j < J; ++j) c4[j] = *reinterpret_cast<const f4*>(p.ln_c1 + ncl[j]);
      }
      if (has_bias) {
#pragma unroll
        for (int j = 0; j < J; ++j) b4[j] = *reinterpret_cast<const f4*>(p.bias + ncl[j]);
      }
      if (rv_one) {
#pragma unroll
        for (int j = 0; j < J; ++j) r4[j] = *reinterpret_cast<const f4*>(p.rowvec + (size_t)b0 * p.ld_rowvec + ncl[j]);
      }
    }
    if constexpr (MODE == EPI_TILE) {
      if (has_res) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < J; ++j) load_res(p, i, j);
      }
    }
  }
  // ahead of outer step o: a row fragment, or (EPI_COLS) a column block
  __device__ __forceinline__ void batch(const IgemmArgs& p, int o, int HoWo) {
    if constexpr (MODE == EPI_COLS) {
      load_col(p, o);
      if (has_rv && !rv_one) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
          rq[i] = *reinterpret_cast<const f4*>(p.rowvec + (size_t)row_sample(p, mcl[i], HoWo) * p.ld_rowvec + ncl[o]);
      }
      if (has_res) {
#pragma unroll
        for (int i = 0; i < MI; ++i) load_res(p, i, o);
      }
    } else {
      if (has_rv && !rv_one) {
        const float* row = p.rowvec + (size_t)row_sample(p, mcl[o], HoWo) * p.ld_rowvec;
#pragma unroll
        for (int j = 0; j < J; ++j) r4[j] = *reinterpret_cast<const f4*>(row + ncl[j]);
      }
      if constexpr (MODE == EPI_ROWS) {
        if (has_res) {
#pragma unroll
          for (int j = 0; j < J; ++j) load_res(p, o, j);
        }
      }
    }
  }
  __device__ __forceinline__ f4 rowvec(int i, int j) const {
    if constexpr (MODE == EPI_COLS) return rv_one ? r4[j] : rq[i];
    return r4[j];
  }
};

// Visits the wave's fragments in the order of MODE: batch(o) ahead of outer step o, elem(i, j) for every fragment, and
// row_done(i) behind the last element of row fragment i.
template <int J, int MI, int MODE, class B, class E, class R>
__device__ __forceinline__ void epi_for_each(B&& batch, E&& elem, R&& row_done) {
  constexpr bool COLS = MODE == EPI_COLS;
#pragma unroll
  for (int o = 0; o < (COLS ? J : MI); ++o) {
    batch(o);
#pragma unroll
    for (int q = 0; q < (COLS ? MI : J); ++q) elem(COLS ? q : o, COLS ? o : q);
    if constexpr (!COLS) row_done(o);
  }
  if constexpr (COLS) {
#pragma unroll
    for (int i = 0; i < MI; ++i) row_done(i);
  }
}

// sum over the 16 lanes of a DPP row (all 16 end up with the total): xor 1, xor 2, half-row mirror, row mirror
__device__ __forceinline__ float dadd_row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
  return v;
}

// The folded upsample conv (UPSF; igemm_ups_fold.hip, 128-row tiles): row `row` of the tile at m0 is input pixel
// (b, y, x) of phase (m0 / BM) & 3 = 2 py + px and is stored at output pixel (2y + py, 2x + px).  -> that pixel's row of `out`
template <int BM>
__device__ __forceinline__ size_t epi_fold_row(const IgemmArgs& p, int m0, int row) {
  const int mt = m0 / BM;
  int b, y, x;
  ups_fold_decode(p, (mt >> 2) * BM + row, b, y, x);
  return ((size_t)(b * p.Ho + 2 * y + ((mt >> 1) & 1))) * p.Wo + 2 * x + (mt & 1);
}

// Every path but GEGLU and the GroupNorm statistics.  FOLD: EPI_PLAIN (also DADD_EPI_LNSTAT), or the LayerNorm folded
// with c1 and the composed bias taken from global memory (EPI_FOLD_GLOBAL: 64-row tiles, whose MFMA waves wait on the
// LDS fill anyway) or staged in LDS at ln_cb (EPI_FOLD_LDS).  The folded linears (qkv, attn2.to_q, the CLIP / resampler
// blocks) have no row partials to write.
enum { EPI_PLAIN = 0, EPI_FOLD_GLOBAL = 1, EPI_FOLD_LDS = 2 };
template <int J, int MI, int WM, int WN, int MODE, int FOLD, bool UPSF = false>
__device__ __forceinline__ void epi_tile(const IgemmArgs& p, f4 (&acc)[J][MI], int m0, int n0, int wm, int wn, int g, int mc,
                                         int HoWo, const float (&lmu)[MI], const float (&lrs)[MI], const char* ln_cb) {
  const bool lnstat = FOLD == EPI_PLAIN && (p.flags & DADD_EPI_LNSTAT) != 0 && n0 + wn * WN < p.N;
  EpiOperands<J, MI, MODE> ops;
  ops.init(p, m0 + wm * WM, n0 + wn * WN, mc, g, HoWo, FOLD != EPI_FOLD_LDS, FOLD == EPI_FOLD_GLOBAL);
  ops.before(p);
  float rs1[MI], rs2[MI];      // DADD_EPI_LNSTAT: this lane's share of row m (J x 4 columns)
#pragma unroll
  for (int i = 0; i < MI; ++i) rs1[i] = rs2[i] = 0.f;
  [[maybe_unused]] size_t orow[MI];      // UPSF: where row fragment i is stored
  if constexpr (UPSF) {
#pragma unroll
    for (int i = 0; i < MI; ++i) orow[i] = epi_fold_row<2 * WM>(p, m0, wm * WM + i * 16 + mc);
  }
  epi_for_each<J, MI, MODE>(
      [&](int o) __attribute__((always_inline)) { ops.batch(p, o, HoWo); },
      [&](int i, int j) __attribute__((always_inline)) {
        const int m = m0 + wm * WM + i * 16 + mc;
        const int c = wn * WN + j * 16 + g * 4, n = n0 + c;
        if (m >= p.M || n >= p.N) return;
        f4 v;
        if constexpr (FOLD == EPI_FOLD_LDS) {
          v = lrs[i] * (acc[j][i] - lmu[i] * *reinterpret_cast<const f4*>(ln_cb + c * 4));
          if (p.flags & DADD_EPI_BIAS) v += *reinterpret_cast<const f4*>(ln_cb + 1024 + c * 4);
        } else if constexpr (FOLD == EPI_FOLD_GLOBAL) {
          v = lrs[i] * (acc[j][i] - lmu[i] * ops.c4[j]) + ops.b4[j];
        } else {
          v = epi_add_if(ops.has_bias, acc[j][i], ops.b4[j]);
        }
        v = epi_add_if(ops.has_rv, v, ops.rowvec(i, j));
        if (p.flags & DADD_EPI_ACT_MASK) epi_activate(p.flags, v);
        v = epi_add_if(ops.has_res, v, ops.res[j][i]);
        h4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          o[r] = (half_t)v[r];
          if constexpr (FOLD == EPI_PLAIN) {
            const float f = (float)o[r];      // statistics of the ROUNDED values, what the consumer multiplies
            rs1[i] += f;
            rs2[i] = fmaf(f, f, rs2[i]);
          }
        }
        if constexpr (UPSF) *reinterpret_cast<h4*>(p.out + orow[i] * p.ldo + n) = o;
        else *reinterpret_cast<h4*>(p.out + (size_t)m * p.ldo + n) = o;
      },
      [&](int i) __attribute__((always_inline)) {
        const int m = m0 + wm * WM + i * 16 + mc;
        if (lnstat && m < p.M) {     // the four lanes (lane & 15) + 16 g hold the WN columns of row m between them
          const float t1 = dadd_sum_x16x32(rs1[i]), t2 = dadd_sum_x16x32(rs2[i]);
          if (g == 0) {
            const int part = (n0 + wn * WN) / WN;
            reinterpret_cast<dadd_f2*>(p.ln_stats_out)[(size_t)part * p.M + m] = dadd_f2{t1, t2};
          }
        }
      });
}

// `ln_mu` / `ln_rs` (MI values each, or nullptr): row mean and 1/std of the folded LayerNorm (igemm_args.h).
// `gn_scratch`: 4 KB of LDS (4 MFMA waves x [80 columns][2] floats) that no LDS-DMA can still be writing when the
// epilogue runs — the staging area of the GroupNorm statistics (DADD_EPI_GNSTAT).
// MODE: EPI_TILE / EPI_ROWS / EPI_COLS above.
// UPSF: the folded upsample conv - rows are stored at epi_fold_row (bias, activation and DADD_EPI_GNSTAT only: resolve).
template <int J, int MI, int WM, int WN, int MODE = EPI_TILE, bool UPSF = false>
__device__ __forceinline__ void igemm_epilogue(const IgemmArgs& p, f4 (&acc)[J][MI], int m0, int n0,
                                               int wm, int wn, int lane, int z, char* smem,
                                               const float* ln_mu = nullptr, const float* ln_rs = nullptr,
                                               char* gn_scratch = nullptr, const char* ln_lds = nullptr,
                                               const char* ln_cb = nullptr) {
  const int g = lane >> 4, mc = lane & 15;
  const int HoWo = p.Ho * p.Wo;
  if (p.splitk > 1) {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int m = m0 + wm * WM + i * 16 + mc;
      if (m >= p.M) continue;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int n = n0 + wn * WN + j * 16 + g * 4;
        if (n < p.N) *reinterpret_cast<f4*>(p.partial + ((size_t)z * p.M + m) * p.N + n) = acc[j][i];
      }
    }
    if (p.counters == nullptr) return;   // combined by splitk_finish_kernel
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                     // every wave's slab stores are issued and drained; LDS is free
    volatile int* flag = reinterpret_cast<volatile int*>(smem);
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      int* ticket = p.counters + blockIdx.x;
      const int prev = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = (prev == p.splitk - 1) ? 1 : 0;
      if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
      }
      *flag = last;
    }
    __syncthreads();
    if (*flag == 0) return;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int m = m0 + wm * WM + i * 16 + mc;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int n = n0 + wn * WN + j * 16 + g * 4;
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (m < p.M && n < p.N)
          for (int s = 0; s < p.splitk; ++s)
            v += *reinterpret_cast<const f4*>(p.partial + ((size_t)s * p.M + m) * p.N + n);
        acc[j][i] = v;
      }
    }
  }
  if (p.flags & DADD_EPI_GNSTAT) {
    // ---- GroupNorm statistics of the OUTPUT from this epilogue: the consumer's gn_stats pass — a full
    // read of the tensor and a launch — disappears.  Host contract: full tiles, Ho*Wo % WM == 0 (a wave's rows lie in
    // one sample), WN % cg == 0 and tile origin aligned to cg (a wave's columns hold whole groups), no split-K.
    // Column-block outer / row-fragment inner, so only one block's partial sums are live beside the accumulators.
    // Sums are taken over the ROUNDED fp16 values (what the consumer reads), in a fixed order: bit-reproducible.
    float* scratch = reinterpret_cast<float*>(gn_scratch) + (wm * 2 + wn) * 256;   // [WN <= 80][2] per wave
    const int mrow0 = m0 + wm * WM;
    // UPSF: the wave's WM rows are input pixels r0 .. r0 + WM of one phase and (Hi*Wi % WM == 0) one sample; they form chunk
    // phase * (Hi*Wi / WM) + (block inside the sample) of its Ho*Wo / WM chunks
    [[maybe_unused]] const int fold_r0 = ((m0 / (2 * WM)) >> 2) * (2 * WM) + wm * WM, fold_ph = (m0 / (2 * WM)) & 3;
    int bsmp;
    if constexpr (UPSF) bsmp = p.fd_on ? (int)dadd_fastdiv_div((uint32_t)fold_r0, p.fd_howo) : fold_r0 / (p.Hi * p.Wi);
    else bsmp = row_sample(p, mrow0, HoWo);
    [[maybe_unused]] size_t orow[MI];
    if constexpr (UPSF) {
#pragma unroll
      for (int i = 0; i < MI; ++i) orow[i] = epi_fold_row<2 * WM>(p, m0, wm * WM + i * 16 + mc);
    }
    const bool has_bias = (p.flags & DADD_EPI_BIAS) != 0, has_rv = (p.flags & DADD_EPI_ROWVEC) != 0;
    const bool has_res = (p.flags & DADD_EPI_RESIDUAL) != 0;
    // the operands of the column blocks (full tiles: nothing to clamp): EPI_TILE all blocks ahead of the first store,
    // else block by block
    f4 b4[J], r4[J];
    h4 res[J][MI];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      b4[j] = r4[j] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < MI; ++i) res[j][i] = h4{};
    }
    auto load_blocks = [&](int ja, int jb) __attribute__((always_inline)) {   // column blocks ja .. jb - 1, one flag test per operand
      const int nw = n0 + wn * WN + g * 4;
      if (has_bias) {
#pragma unroll
        for (int j = 0; j < J; ++j)
          if (j >= ja && j < jb) b4[j] = *reinterpret_cast<const f4*>(p.bias + nw + j * 16);
      }
      if (has_rv) {
#pragma unroll
        for (int j = 0; j < J; ++j)
          if (j >= ja && j < jb) r4[j] = *reinterpret_cast<const f4*>(p.rowvec + (size_t)bsmp * p.ld_rowvec + nw + j * 16);
      }
      if (has_res) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < J; ++j)
            if (j >= ja && j < jb)
              res[j][i] = *reinterpret_cast<const h4*>(p.residual + (size_t)(mrow0 + i * 16 + mc) * p.ldr + nw + j * 16);
      }
    };
    if constexpr (MODE == EPI_TILE) load_blocks(0, J);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int n = n0 + wn * WN + j * 16 + g * 4;
      if constexpr (MODE != EPI_TILE) load_blocks(j, j + 1);
      f4 bias4 = {0.f, 0.f, 0.f, 0.f};
      if (has_bias) bias4 = b4[j];
      bias4 = epi_add_if(has_rv, bias4, r4[j]);
      float cs[4] = {0.f, 0.f, 0.f, 0.f}, cq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int m = mrow0 + i * 16 + mc;
        f4 v = acc[j][i] + bias4;
        v = epi_add_if(has_res, v, res[j][i]);
        h4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          o[r] = (half_t)v[r];
          const float f = (float)o[r];
          cs[r] += f;
          cq[r] = fmaf(f, f, cq[r]);
        }
        if constexpr (UPSF) *reinterpret_cast<h4*>(p.out + orow[i] * p.ldo + n) = o;
        else *reinterpret_cast<h4*>(p.out + (size_t)m * p.ldo + n) = o;
      }
      // 16 lanes (mc) share a column quad: butterfly inside the DPP row (quad perms, half mirror, mirror)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        cs[r] = dadd_row16_sum(cs[r]);
        cq[r] = dadd_row16_sum(cq[r]);
      }
      if (mc == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          scratch[(j * 16 + g * 4 + r) * 2] = cs[r];
          scratch[(j * 16 + g * 4 + r) * 2 + 1] = cq[r];
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int ngrp = WN / p.gn_cg;
    if (lane < ngrp) {
      float a = 0.f, q = 0.f;
      for (int c = 0; c < p.gn_cg; ++c) {
        a += scratch[(lane * p.gn_cg + c) * 2];
        q += scratch[(lane * p.gn_cg + c) * 2 + 1];
      }
      int chunk;
      if constexpr (UPSF) chunk = (fold_ph * (p.Hi * p.Wi) + fold_r0 - bsmp * (p.Hi * p.Wi)) / WM;
      else chunk = (mrow0 - bsmp * HoWo) / WM;
      const int grp = (n0 + wn * WN) / p.gn_cg + lane;
      float* w = p.gn_ws + (((size_t)bsmp * p.gn_nchunk + chunk) * 32 + grp) * 2;
      w[0] = a;
      w[1] = q;
    }
    return;
  }
  // ---- folded LayerNorm.  Row mean / rstd either come from the caller (the LDS-DMA kernel summed the rows of its A
  // fragments) or from the GEMM that produced x (its DADD_EPI_LNSTAT): ln_parts_in float2 partials per row, lanes of
  // a 16-lane row read 16 consecutive rows (128 B); four parts x MI rows are in flight together.
  // (plain register arrays, filled by fully unrolled code: selecting between two arrays through a pointer would put
  // them in scratch)
  float lmu[MI], lrs[MI];
  bool fold = false;
  if (ln_mu != nullptr) {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      lmu[i] = ln_mu[i];
      lrs[i] = ln_rs[i];
    }
    fold = true;
  } else if ((p.flags & DADD_EPI_LNFOLD) && p.ln_stats_in != nullptr) {
    const dadd_f2* st = reinterpret_cast<const dadd_f2*>(p.ln_stats_in);
    float sa[MI], sq[MI];
    int mrow[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      sa[i] = sq[i] = 0.f;
      mrow[i] = min(m0 + wm * WM + i * 16 + mc, p.M - 1);
    }
    if (ln_lds != nullptr) {            // staged in LDS by ln_lds_issue(): [part][tile row][2]
      for (int pp = 0; pp < p.ln_parts_in; ++pp)
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          const dadd_f2 v = *reinterpret_cast<const dadd_f2*>(ln_lds + pp * 1024 + (wm * WM + i * 16 + mc) * 8);
          sa[i] += v[0];
          sq[i] += v[1];
        }
    } else
    for (int pp = 0; pp < p.ln_parts_in; pp += 4) {
      dadd_f2 v[4][MI];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < MI; ++i)
          v[u][i] = st[(size_t)min(pp + u, p.ln_parts_in - 1) * p.M + mrow[i]];   // unconditional: no branch, no wait per load
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float keep = (pp + u < p.ln_parts_in) ? 1.f : 0.f;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          sa[i] = fmaf(keep, v[u][i][0], sa[i]);
          sq[i] = fmaf(keep, v[u][i][1], sq[i]);
        }
      }
    }
    const float inv = __builtin_amdgcn_rcpf((float)p.K);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const float mu = sa[i] * inv;
      lmu[i] = mu;
      lrs[i] = rsqrtf(fmaxf(epi_ln_var(epi_ln_var_fused(J, MI, i), sq[i] * inv, mu), 0.f) + p.ln_eps);
    }
    fold = true;
  } else {
#pragma unroll
    for (int i = 0; i < MI; ++i) lmu[i] = 0.f, lrs[i] = 1.f;
  }
  const bool lds_fold = fold && ln_cb != nullptr;
  if (lds_fold && (p.flags & DADD_EPI_GEGLU)) {
    // ---- folded LayerNorm + GEGLU, c1 and the composed bias staged in LDS: no operand in global memory
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int m = m0 + wm * WM + i * 16 + mc;
      if (m >= p.M) continue;
      if constexpr (J == 4) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int ch = wn * WN + j * 16 + g * 4, cg2 = ch + 32;      // tile-relative columns: hidden, gate
          if (n0 + cg2 >= p.N) continue;
          f4 hv = lrs[i] * (acc[j][i] - lmu[i] * *reinterpret_cast<const f4*>(ln_cb + ch * 4));
          f4 gv = lrs[i] * (acc[j + 2][i] - lmu[i] * *reinterpret_cast<const f4*>(ln_cb + cg2 * 4));
          if (p.flags & DADD_EPI_BIAS) {
            hv += *reinterpret_cast<const f4*>(ln_cb + 1024 + ch * 4);
            gv += *reinterpret_cast<const f4*>(ln_cb + 1024 + cg2 * 4);
          }
          const int no = (n0 >> 1) + wn * 32 + j * 16 + g * 4;
          const dadd_f2 g01 = dadd_gelu2(dadd_f2{gv[0], gv[1]}), g23 = dadd_gelu2(dadd_f2{gv[2], gv[3]});
          const h4 o = {(half_t)(hv[0] * g01[0]), (half_t)(hv[1] * g01[1]), (half_t)(hv[2] * g23[0]),
                        (half_t)(hv[3] * g23[1])};
          *reinterpret_cast<h4*>(p.out + (size_t)m * p.ldo + no) = o;
        }
      }
    }
    return;
  }
  if (p.flags & DADD_EPI_GEGLU) {
    // ---- GEGLU, plain or with the LayerNorm folded from global operands (64-row tiles, whose MFMA waves wait on the
    // LDS fill anyway).  Physical (interleaved) weight rows: the gate of column block j is block j + 2.  The c1 and
    // bias quads of the four blocks are loaded ahead of the rows (EPI_COLS: those of a hidden block and its gate ahead
    // of that block's rows).
    if constexpr (J == 4) {
      const bool has_bias = (p.flags & DADD_EPI_BIAS) != 0;
      auto geglu = [&](auto folded) __attribute__((always_inline)) {
        constexpr bool FOLD = decltype(folded)::value, COLS = MODE == EPI_COLS;
        f4 c1[J], b4[J];
#pragma unroll
        for (int j = 0; j < J; ++j) c1[j] = b4[j] = f4{0.f, 0.f, 0.f, 0.f};
        auto load_pair = [&](int j) __attribute__((always_inline)) {      // hidden block j and its gate
          const int nh = min(n0 + wn * WN + j * 16 + g * 4, p.N - 4), ng = min(n0 + wn * WN + j * 16 + g * 4 + 32, p.N - 4);
          if constexpr (FOLD) {
            c1[j] = *reinterpret_cast<const f4*>(p.ln_c1 + nh);
            c1[j + 2] = *reinterpret_cast<const f4*>(p.ln_c1 + ng);
          }
          if (has_bias) {
            b4[j] = *reinterpret_cast<const f4*>(p.bias + nh);
            b4[j + 2] = *reinterpret_cast<const f4*>(p.bias + ng);
          }
        };
        if constexpr (!COLS) {
          load_pair(0);
          load_pair(1);
        }
#pragma unroll
        for (int o = 0; o < (COLS ? 2 : MI); ++o) {
          if constexpr (COLS) load_pair(o);
#pragma unroll
          for (int q = 0; q < (COLS ? MI : 2); ++q) {
            const int i = COLS ? q : o, j = COLS ? o : q;
            const int m = m0 + wm * WM + i * 16 + mc;
            if (m >= p.M || n0 + wn * WN + j * 16 + g * 4 + 32 >= p.N) continue;
            f4 hv, gv;
            if constexpr (FOLD) {
              hv = lrs[i] * (acc[j][i] - lmu[i] * c1[j]) + b4[j];
              gv = lrs[i] * (acc[j + 2][i] - lmu[i] * c1[j + 2]) + b4[j + 2];
            } else {
              hv = epi_add_if(has_bias, acc[j][i], b4[j]);
              gv = epi_add_if(has_bias, acc[j + 2][i], b4[j + 2]);
            }
            const int no = (n0 >> 1) + wn * 32 + j * 16 + g * 4;
            const dadd_f2 g01 = dadd_gelu2(dadd_f2{gv[0], gv[1]}), g23 = dadd_gelu2(dadd_f2{gv[2], gv[3]});
            const h4 o4 = {(half_t)(hv[0] * g01[0]), (half_t)(hv[1] * g01[1]), (half_t)(hv[2] * g23[0]),
                           (half_t)(hv[3] * g23[1])};
            *reinterpret_cast<h4*>(p.out + (size_t)m * p.ldo + no) = o4;
          }
        }
      };
      if (fold) geglu(std::true_type{});
      else geglu(std::false_type{});
    }
    return;
  }
  if constexpr (UPSF) {
    epi_tile<J, MI, WM, WN, MODE, EPI_PLAIN, true>(p, acc, m0, n0, wm, wn, g, mc, HoWo, lmu, lrs, ln_cb);
    return;
  }
  if (lds_fold) epi_tile<J, MI, WM, WN, MODE, EPI_FOLD_LDS>(p, acc, m0, n0, wm, wn, g, mc, HoWo, lmu, lrs, ln_cb);
  else if (fold) epi_tile<J, MI, WM, WN, MODE, EPI_FOLD_GLOBAL>(p, acc, m0, n0, wm, wn, g, mc, HoWo, lmu, lrs, ln_cb);
  else epi_tile<J, MI, WM, WN, MODE, EPI_PLAIN>(p, acc, m0, n0, wm, wn, g, mc, HoWo, lmu, lrs, ln_cb);
}
