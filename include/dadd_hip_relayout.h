/*
 * dadd_hip_relayout.h - the part of libdadd_hip.so's C ABI that re-lays the 16-bit working copy of the weights for the
 * data gradients of a training step (csrc/relayout.hip and its bf16 twin).  Conventions and status codes are those of
 * dadd_hip.h.
 *
 * The data gradient of every matrix product reads its weight in a second layout (grad_ops.dgrad_weight and its
 * siblings).  One launch of dadd_dgrad_relayout_* writes that layout for every listed tensor: it reads `src`, a flat
 * 16-bit array (the optimizer's p16), and writes `dst`, a second flat 16-bit array.  A device-resident table of
 * dadd_relayout_desc says where each tensor lives in both and what kind of re-layout it gets.  The kernel moves whole
 * values and, for the UPS kind, adds in a fixed order: a call repeated on the same operands gives the same bits.
 *
 * A tensor is the library layout [N][taps][C] (taps 1 or 9).  Its kinds, with slab s of the destination row:
 *   DADD_RELAYOUT_T      dst [C][taps][N]:  dst[c][s][n] = src[n][taps - 1 - s][c]        (grad_ops.dgrad_weight)
 *   DADD_RELAYOUT_S2     dst [C][9][N]:     dst[c][s][n] = src[n][tap(s)][c], tap(s) = 4,3,5,1,7,0,2,6,8: the slabs of
 *                                           the parity classes of dadd_hip_dgrad.h      (grad_ops.dgrad_weight_stride2)
 *   DADD_RELAYOUT_UPS    dst [C][16][N]:    dst[c][4e + f][n] = round16((sum over ky in S(e) of src[n][ky][kx0][c]) +
 *                                           (the same sum at kx1)), S(0..3) = {2}, {1,2}, {0,1}, {0}, kx in S(f); the
 *                                           sums run in fp32, ky first, then kx, one rounding (grad_ops.dgrad_weight_ups)
 *   DADD_RELAYOUT_COUT4  src [N <= 4][9][C], dst [C][9][8]: dst[c][s][o] = src[o][8 - s][c] for o < N, 0 for o >= N
 *                                                                                        (grad_ops.dgrad_weight_cout4)
 * Contract of a descriptor: src_off and dst_off multiples of 8 elements and >= 0; C a positive multiple of 8; N a
 * positive multiple of 8 (COUT4: 1..4); taps 1 or 9 for T, 9 for every other kind.  The kernel needs no size to be a
 * multiple of its 64 x 64 tile.
 *
 * Workgroup w of the launch works on tile w - tile0 of the last descriptor whose tile0 is <= w: tile0 is the running
 * sum of dadd_relayout_tiles over the table, which dadd_dgrad_relayout_plan fills in.
 */
#ifndef DADD_HIP_RELAYOUT_H
#define DADD_HIP_RELAYOUT_H

#include "dadd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DADD_RELAYOUT_T 0
#define DADD_RELAYOUT_S2 1
#define DADD_RELAYOUT_UPS 2
#define DADD_RELAYOUT_COUT4 3
#define DADD_RELAYOUT_TILE 64 /* a tile is 64 n x 64 c of one destination slab (COUT4: 256 (c, slab) pairs) */

typedef struct dadd_relayout_desc {
  long long src_off; /* elements from `src` to the tensor */
  long long dst_off; /* elements from `dst` to its re-laid copy */
  int N, C, kind, taps;
  int tile0;         /* out of dadd_dgrad_relayout_plan: the first workgroup of this tensor */
  int reserved;
} dadd_relayout_desc;

/* Number of tiles (workgroups) of one tensor, -1 when (kind, taps, N, C) breaks the contract.  Host only. */
long long dadd_relayout_tiles(int kind, int taps, int N, int C);

/* Number of elements of the re-laid copy of one tensor, -1 when (kind, taps, N, C) breaks the contract.  Host only. */
long long dadd_relayout_dst_numel(int kind, int taps, int N, int C);

/* Checks every descriptor of the HOST array `descs` [n] against the contract and against the two array lengths (every
 * source and destination range inside its array, no two destination ranges overlapping when the table is in ascending
 * dst_off order, which it must be), writes tile0 and returns the total number of tiles: the grid of the launch.
 * Returns -1 with dadd_last_error() set otherwise.  Host only, no GPU involved. */
long long dadd_dgrad_relayout_plan(dadd_relayout_desc* descs, int n, long long src_numel, long long dst_numel);

/* One launch of n_tiles workgroups of 256 lanes: `table` is the DEVICE copy of a planned descriptor array [n_desc],
 * n_tiles the plan's return value.  src [src_numel] and dst [dst_numel] are 16-bit arrays, 16-byte aligned.  A workgroup
 * whose descriptor does not fit the two lengths writes nothing.  Elements of dst outside the listed ranges are not
 * touched. */
int dadd_dgrad_relayout_f16(const void* src, long long src_numel, void* dst, long long dst_numel,
                            const dadd_relayout_desc* table, int n_desc, int n_tiles, void* stream);
int dadd_dgrad_relayout_bf16(const void* src, long long src_numel, void* dst, long long dst_numel,
                             const dadd_relayout_desc* table, int n_desc, int n_tiles, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DADD_HIP_RELAYOUT_H */
