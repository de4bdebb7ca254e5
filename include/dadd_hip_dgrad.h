/*
 * dadd_hip_dgrad.h - the part of libdadd_hip.so's C ABI that carries the data gradient of the two resampling 3x3
 * convolutions of the UNet (csrc/dgrad.hip, bf16 twin csrc/dgrad_bf16.hip): stride 2 (diffusers' Downsample2D) and
 * nearest-2x-upsample-then-conv (Upsample2D).  The stride-1 data gradient needs no entry point of its own: it is the
 * forward GEMM on dy with a re-laid weight (dadd_hip.h).  Conventions and status codes are those of dadd_hip.h: NHWC
 * tensors in the 16-bit type of the suffix (_f16 or _bf16, same argument list), the call launches on `stream` and returns
 * DADD_OK, DADD_EINVAL (contract, see dadd_last_error(); nothing has been launched then) or DADD_EHIP.  One launch, no
 * atomics, no split of the reduction: a call repeated on the same operands gives the same bits.
 *
 * The algebra.  Sizes are those of the FORWARD conv: x [B][Hi][Wi][C] -> y [B][Ho][Wo][N], padding 1.
 *   STRIDE2: input pixel (2 jy + py, 2 jx + px) of parity class (py, px) receives only the taps whose source is an
 *     integer output pixel: py = 0: ky = 1 from oy = jy; py = 1: ky = 0 from oy = jy + 1 and ky = 2 from oy = jy; the same
 *     in x.  Classes (0,0), (0,1), (1,0), (1,1) have 1, 2, 2 and 4 taps; sources with oy >= Ho or ox >= Wo are zero.
 *     `wt` holds the 9 weight slabs in CLASS ORDER, as (ky, kx):
 *         (1,1) | (1,0) (1,2) | (0,1) (2,1) | (0,0) (0,2) (2,0) (2,2)
 *     so the slabs of one class are adjacent and a class's K = ntaps * N is one run; the source of slab (ky, kx) is
 *     (jy + (ky == 0), jx + (kx == 0)).
 *   UPS: dx[iy][ix] = sum over e, f in {-1, 0, 1, 2} of dy[2 iy + e][2 ix + f] . W4[e][f], with
 *     W4[e][f] = sum of w[ky][kx] over ky in S(e), kx in S(f), S(-1) = {2}, S(0) = {1, 2}, S(1) = {0, 1}, S(2) = {0}
 *     (the caller sums in fp32 and rounds once to the operand type): one class of 16 taps, slab 4 (e + 1) + (f + 1);
 *     rows outside [0, 2 Hi) and columns outside [0, 2 Wi) are zero.
 */
#ifndef DADD_HIP_DGRAD_H
#define DADD_HIP_DGRAD_H

#include <stdint.h>

#include "dadd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DADD_DGRAD_STRIDE2 0
#define DADD_DGRAD_UPS     1
#define DADD_DGRAD_MAX_CLASSES 4

typedef struct {
  const void* dy;   /* [B][Ho][Wo][N] 16-bit, ld_dy between pixels */
  const void* wt;   /* [C][T*N] 16-bit, T = 9 (stride 2, class order) or 16 (ups, summed) */
  void* dx;         /* [B][Hi][Wi][C] 16-bit, ld_dx between pixels; overwritten, every pixel */
  int32_t B, Hi, Wi, C, Ho, Wo, N;   /* of the FORWARD conv */
  int32_t mode, ld_dy, ld_dx;
} dadd_dgrad_desc;

/* One class of output pixels: the pixels (jy * so + py, jx * so + px) of every sample, so = 2 (STRIDE2) or 1 (UPS), in
 * the order (b, jy, jx); the class owns the tiles [first_tile, first_tile + ceil(pixels / 64)) of grid_x and reduces over
 * the weight slabs [first_slab, first_slab + ntaps). */
typedef struct {
  int32_t first_tile, pixels, py, px, first_slab, ntaps;
} dadd_dgrad_class;

/* What dadd_conv_dgrad_* launches for a descriptor. */
typedef struct {
  int32_t grid_x, grid_y;   /* (sum over classes of ceil(pixels / 64), C / 64) */
  int32_t block;            /* threads per workgroup */
  int32_t smem;             /* bytes of LDS per workgroup */
  int32_t nclass;           /* classes with at least one pixel, <= DADD_DGRAD_MAX_CLASSES */
  int32_t xcd_by_c;         /* 1: workgroups renumbered so that an XCD's L2 sees a run of c tiles (the weight is the
                             * larger operand and grid_x * grid_y is a multiple of 8); 0: launch order.  Placement only. */
  dadd_dgrad_class cls[DADD_DGRAD_MAX_CLASSES];
} dadd_dgrad_choice;

/* dx = the gradient of the forward conv with respect to x, rounded once to the 16-bit type; fp32 accumulation.
 * Contract: C % 64 == 0, N % 8 == 0; ld_dy >= N and ld_dx >= C, both multiples of 8; pointers non-NULL and 16-byte
 * aligned; every size positive; mode STRIDE2 with Ho == (Hi - 1) / 2 + 1 and Wo == (Wi - 1) / 2 + 1, or mode UPS with
 * Ho == 2 Hi and Wo == 2 Wi; fewer than 2^31 pixels in dy and in dx.  dx must not alias dy or wt.  Every pixel of dx is
 * written, C columns of it; columns outside are left untouched. */
int dadd_conv_dgrad_f16(const dadd_dgrad_desc* d, void* stream);
int dadd_conv_dgrad_bf16(const dadd_dgrad_desc* d, void* stream);

/* Host only: the validation and the decisions of the launch (either 16-bit type) without the launch.  Makes no HIP call
 * and reads no buffer; the launchers call this same function. */
int dadd_conv_dgrad_resolve(const dadd_dgrad_desc* d, dadd_dgrad_choice* out);

#ifdef __cplusplus
}
#endif
#endif /* DADD_HIP_DGRAD_H */
