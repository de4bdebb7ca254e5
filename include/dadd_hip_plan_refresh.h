/*
 * dadd_hip_plan_refresh.h - the part of libdadd_hip.so's C ABI that rewrites the packed weights of live inference plans
 * from a flat array of fp32 masters (csrc/plan_refresh.hip and its bf16 twin): the forward-direction sibling of
 * dadd_hip_relayout.h.  Conventions and status codes are those of dadd_hip.h.
 *
 * A plan keeps every weight as a persistent device tensor in the layout its kernel reads (engine.py: pack_conv,
 * geglu_interleave, fold_layernorm, fold_ups_weight, pack_head_stream, pack_ffn_stream).  One launch of
 * dadd_plan_refresh_* writes all of them again from `src`, one flat fp32 array (the optimizer's p or its EMA).  A
 * device-resident table of dadd_plan_refresh_desc says where each source lives in `src`, what kind of packing it gets
 * and where the result goes: destinations are the plan's own tensors, so a descriptor carries pointers.  No atomics;
 * every sum has a fixed order: a call repeated on the same operands gives the same bits.
 *
 * Sources are the library layout [N][taps * C] fp32.  "16" below is the 16-bit type of the entry point (fp16 or bf16);
 * every conversion to it rounds to nearest even.  Kinds (N, K, Cs are the descriptor's fields):
 *   COPY32       dst0 fp32 [N]           = src0 [N]
 *   CAST         dst0 16 [N][K]          = src0 [N][Cs], Cs == K; or K == 8 and 1 <= Cs < 8: every row of Cs values is
 *                                          zero-padded to 8 (pack_conv_cin8 with N = Cout * 9).  A row concatenation is
 *                                          several descriptors whose dst0 point into one tensor.
 *   GEGLU_W      dst0 16 [N][K]          row r = src0 row g(r), g = geglu_interleave's order: r = 128 t + 64 wn + q ->
 *                                          64 t + 32 wn + q % 32, plus N / 2 when q >= 32
 *   GEGLU_B      dst0 fp32 [N]           dst0[r] = src0[g(r)]
 *   LNFOLD       fold_layernorm: src0 = W [N][K], src1 = gamma [K], src2 = beta [K], src3 = b [N] or -1;
 *                dst0 16 [N][K], dst1 fp32 [N] (c1), dst2 fp32 [N] (bias).  With s = g(r) under DADD_PLAN_REFRESH_GEGLU,
 *                else s = r:   dst0[r][k] = round16(round32(W[s][k] * gamma[k]))
 *                              dst1[r]    = round32(sum_k (double)dst0[r][k])
 *                              dst2[r]    = round32(sum_k (double)W[s][k] * (double)beta[k] + b[s])
 *                Products and sums in fp64.  One wave per row: lane l adds its elements k = 8 l + 512 j + e in ascending
 *                order, then the 64 lane sums meet in a butterfly (lane distance 32, 16, .. 1).
 *   UPSFOLD      fold_ups_weight: src0 [N][9][K] -> dst0 16 [4][N][4][K].  Phase 2 py + px, tap 2 dy + dx sums the taps
 *                (ky, kx), ky in S(py, dy), kx in S(px, dx), S(0, 0) = {0}, S(0, 1) = {1, 2}, S(1, 0) = {0, 1},
 *                S(1, 1) = {2}: each tap rounded to 16 first, the sum in fp64 (ky outer), then round32, then round16.
 *   HEAD_STREAM  pack_head_stream: src0..3 = proj_in, to_q, to_k, to_v, each [320][320] -> dst0 16 [409600]
 *   FFN_STREAM   pack_ffn_stream: src0 = ff.net.0.proj [2560][320], src1 = ff.net.2 [320][1280], src2 = proj_out
 *                [320][320] -> dst0 16 [1331200]
 *   FFN_BIAS     the permuted GEGLU bias of pack_ffn_stream: src0 [2560] -> dst0 fp32 [2560]
 * The two stream kinds and FFN_BIAS need K == 320.
 *
 * Contract of a descriptor.  Every source range lies inside [0, src_numel); every dst_room (elements of the
 * destination's own type that may be written from that pointer on) covers what the kind writes.  COPY32, GEGLU_B and
 * FFN_BIAS: N >= 1, pointers 4-byte aligned.  Every other kind: dst0 16-byte aligned, the source offsets multiples of 4
 * elements (the padded CAST: any), N * K (CAST) resp. K (others) a multiple of 8, dst1 / dst2 4-byte aligned; GEGLU_W,
 * GEGLU_B and LNFOLD in GEGLU order: N a multiple of 128.  No two destination ranges of a table overlap.
 *
 * Workgroup w of the launch works on unit w - wg0 of the last descriptor whose wg0 is <= w: wg0 is the running sum of
 * dadd_plan_refresh_wgs over the table, which dadd_plan_refresh_plan fills in.
 */
#ifndef DADD_HIP_PLAN_REFRESH_H
#define DADD_HIP_PLAN_REFRESH_H

#include "dadd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DADD_PLAN_REFRESH_COPY32 0
#define DADD_PLAN_REFRESH_CAST 1
#define DADD_PLAN_REFRESH_GEGLU_W 2
#define DADD_PLAN_REFRESH_GEGLU_B 3
#define DADD_PLAN_REFRESH_LNFOLD 4
#define DADD_PLAN_REFRESH_UPSFOLD 5
#define DADD_PLAN_REFRESH_HEAD_STREAM 6
#define DADD_PLAN_REFRESH_FFN_STREAM 7
#define DADD_PLAN_REFRESH_FFN_BIAS 8

#define DADD_PLAN_REFRESH_GEGLU 1 /* flags: LNFOLD writes its rows in GEGLU order */

#define DADD_PLAN_REFRESH_GROUPS 1024 /* a workgroup writes 1024 groups of 8 16-bit values, ... */
#define DADD_PLAN_REFRESH_SCALARS 2048 /* ... 2048 fp32 values of the fp32 kinds, ... */
#define DADD_PLAN_REFRESH_ROWS 4       /* ... or 4 rows of LNFOLD, one per wave */

typedef struct dadd_plan_refresh_desc {
  long long src_off[4];  /* elements from `src` to each source; -1 = absent */
  void* dst[3];          /* device pointers; dst[1], dst[2]: LNFOLD's c1 and bias */
  long long dst_room[3]; /* elements that may be written at each dst */
  int kind, N, K, Cs;
  int flags;
  int wg0; /* out of dadd_plan_refresh_plan: the first workgroup of this descriptor */
  int reserved[2];
} dadd_plan_refresh_desc;

/* Number of workgroups of one descriptor, -1 when (kind, N, K, Cs, flags) breaks the contract.  Host only. */
long long dadd_plan_refresh_wgs(int kind, int N, int K, int Cs, int flags);

/* Checks every descriptor of the HOST array `descs` [n] against the contract (sizes, alignment, every source range
 * inside [0, src_numel), every dst_room large enough, no two destination ranges overlapping), writes wg0 and returns the
 * total number of workgroups: the grid of the launch.  Returns -1 with dadd_last_error() set otherwise.  Host only: the
 * destination pointers are compared, never dereferenced. */
long long dadd_plan_refresh_plan(dadd_plan_refresh_desc* descs, int n, long long src_numel);

/* One launch of n_wgs workgroups of 256 lanes: `table` is the DEVICE copy of a planned descriptor array [n_desc], n_wgs
 * the plan's return value; src [src_numel] is fp32, 16-byte aligned.  A workgroup whose descriptor does not fit src_numel,
 * its dst_room or the contract of its kind writes nothing.  Memory outside the listed destination ranges is not touched. */
int dadd_plan_refresh_f16(const void* src, long long src_numel, const dadd_plan_refresh_desc* table, int n_desc,
                          int n_wgs, void* stream);
int dadd_plan_refresh_bf16(const void* src, long long src_numel, const dadd_plan_refresh_desc* table, int n_desc,
                           int n_wgs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DADD_HIP_PLAN_REFRESH_H */
