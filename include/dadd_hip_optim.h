/*
 * dadd_hip_optim.h - the part of libdadd_hip.so's C ABI that carries the optimizer of a training step: global-norm
 * gradient clipping, the loss scale with skip-on-overflow, AdamW over up to DADD_OPTIM_MAX_GROUPS parameter groups, the
 * EMA of the weights, the 16-bit working copy of the weights and the zeroing of the gradients (csrc/optim.hip; one
 * source, the 16-bit type of the working copy is a flag).  Conventions and status codes are those of dadd_hip.h: plain
 * pointers, sizes and `stream`; every call returns DADD_OK or DADD_EINVAL (contract, see dadd_last_error(); nothing has
 * been launched then) or DADD_EHIP.  The kernels use no atomics: every sum runs in a fixed order and a call repeated on
 * the same operands gives the same bits.
 *
 * All parameter state lives in flat fp32 arrays of one common length n, a multiple of DADD_OPTIM_CHUNK: p (master
 * weights), g (gradients), m and v (the moments), optionally ema, and optionally p16 (n 16-bit elements).  A chunk is
 * DADD_OPTIM_CHUNK consecutive elements; one workgroup of 256 lanes moves it with four 16-byte loads per lane and array.
 * Every group is a whole number of chunks, so a workgroup never straddles two groups.
 *
 * One optimizer step is three launches on one stream, with no host involvement in between:
 *   dadd_optim_grad_stats -> dadd_optim_finalize -> dadd_optim_adamw_step
 * The host writes the learning rates into the state block between steps and nothing else after construction, so a
 * captured graph of the three launches replays across a whole schedule.
 */
#ifndef DADD_HIP_OPTIM_H
#define DADD_HIP_OPTIM_H

#include "dadd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DADD_OPTIM_CHUNK 4096
#define DADD_OPTIM_MAX_GROUPS 8

/* flags of dadd_optim_adamw_step */
#define DADD_OPTIM_EMA 1       /* ema = ema + (p_new - ema) * ema_weight */
#define DADD_OPTIM_P16_F16 2   /* p16 = (fp16)p_new, round to nearest even */
#define DADD_OPTIM_P16_BF16 4  /* p16 = (bf16)p_new, round to nearest even; excludes DADD_OPTIM_P16_F16 */
#define DADD_OPTIM_ZERO_GRAD 8 /* g = 0 */

/* One parameter group: 12 floats.  The first six are the host's, written at construction; the next three are written by
 * dadd_optim_finalize for the step it has just counted.  one_minus_beta1 / 2 are 1 - beta rounded to fp32 from the
 * host's double: beta itself rounded to fp32 would leave 1 - beta2 = 0.001 with a relative error of 3e-5, and the bias
 * correction of the first steps with it.  The powers are taken of 1 - (double)one_minus_beta. */
typedef struct dadd_optim_group {
  float beta1, beta2, eps, weight_decay, one_minus_beta1, one_minus_beta2;
  float decay;     /* 1 - lr * weight_decay */
  float step_size; /* lr / (1 - beta1^t) */
  float rsqrt_bc2; /* 1 / sqrt(1 - beta2^t) */
  float reserved[3];
} dadd_optim_group;

/* The device-resident state block: 16 four-byte words, the learning rates (contiguous: the one thing the host rewrites
 * between steps, with one small copy), then the groups: 16 + 13 * DADD_OPTIM_MAX_GROUPS words. */
typedef struct dadd_optim_state {
  int step;            /* t: number of steps applied; a skipped step does not count */
  int found_inf;       /* out: 1 when the last dadd_optim_finalize saw a non-finite gradient */
  int growth_tracker;  /* consecutive clean steps since the last change of the scale */
  int growth_interval; /* host: clean steps after which the scale grows */
  int n_groups;        /* host: 1 .. DADD_OPTIM_MAX_GROUPS */
  int reserved_i[3];
  float grad_norm;     /* out: sqrt(sum g^2) / scale, the norm of the unscaled gradient */
  float coef;          /* out: what the step multiplies g by; 0 on a skipped step */
  float scale;         /* the loss scale; 0 on entry = no loss scaling (never updated then) */
  float max_norm;      /* host: clip threshold; <= 0 disables clipping */
  float growth_factor; /* host */
  float backoff_factor;/* host */
  float reserved_f[2];
  float lr[DADD_OPTIM_MAX_GROUPS]; /* host: the rate of each group for the next step */
  dadd_optim_group group[DADD_OPTIM_MAX_GROUPS];
} dadd_optim_state;

/* One pass over g [n]: partials[c] = sum of g^2 over chunk c (each lane adds its 16 squares in fp32 in index order, then
 * a fixed-order wave and workgroup reduction: 15 + 6 + 3 = 24 additions deep) and flags[c] = 1 when any value of the
 * chunk is inf or NaN, else 0.  Partial and flag belong to the chunk, not to the workgroup that processed it: the result
 * does not depend on the grid.  The grid is min(n / DADD_OPTIM_CHUNK, max_blocks) workgroups striding over the chunks;
 * max_blocks = 0 takes the kernel's default.  Contract: n > 0 a multiple of DADD_OPTIM_CHUNK with at most 2^31 - 1
 * chunks, g 16-byte aligned, max_blocks >= 0. */
int dadd_optim_grad_stats(const float* g, long long n, float* partials, int* flags, int max_blocks, void* stream);

/* One workgroup, all the scalar work of a step.  Reads partials / flags [n_chunks] (each of its 1024 lanes its strided
 * share in index order, then a fixed tree over the lanes), sums in double, and updates *state:
 *   found_inf = any flag;   inv_scale = scale == 0 ? 1 : 1 / scale;   grad_norm = sqrt(sum) * inv_scale
 *   coef      = found_inf ? 0 : inv_scale * (max_norm > 0 ? min(1, max_norm / (grad_norm + 1e-6)) : 1)
 *   clean step: step += 1, and per group from the new step t (powers in double)
 *               decay = 1 - lr * weight_decay, step_size = lr / (1 - beta1^t), rsqrt_bc2 = 1 / sqrt(1 - beta2^t)
 *   scale (when not 0), torch.amp.GradScaler's rule: overflow -> scale *= backoff_factor, growth_tracker = 0; else
 *               growth_tracker += 1, and at growth_interval scale *= growth_factor, growth_tracker = 0.
 * On overflow nothing but found_inf, grad_norm, coef, scale and growth_tracker changes.  Contract: n_chunks in
 * 1 .. 2^31 - 1, non-null pointers. */
int dadd_optim_finalize(const float* partials, const int* flags, long long n_chunks, dadd_optim_state* state,
                        void* stream);

/* One pass over the arena.  Per element, with the constants of the chunk's group and c = state->coef, every operation
 * rounded to fp32 in this order (IEEE sqrt and division, no fused multiply-add):
 *   g' = g * c;  p = p * decay;  m = m + (g' - m) * one_minus_beta1;  v = v * beta2 + (g' * g') * one_minus_beta2
 *   p = p - step_size * (m / (sqrt(v) * rsqrt_bc2 + eps))
 * With state->found_inf set p, m and v are left as they are.  Then, by `flags`, on the new (or untouched) p: the EMA
 * with ema_weight = 1 - decay of the average, the 16-bit copy, and g = 0; these run on a skipped step too.
 * group_chunks [n_groups] is a HOST array: the number of chunks of each group, in arena order; it must sum to
 * n / DADD_OPTIM_CHUNK and n_groups must equal state->n_groups (the caller's business: the block is on the device).
 * Contract: as dadd_optim_grad_stats, all arrays 16-byte aligned (p16: 8-byte), ema given exactly when DADD_OPTIM_EMA is
 * set, p16 exactly with one of the two P16 flags, 1 <= n_groups <= DADD_OPTIM_MAX_GROUPS, every group_chunks[k] >= 0. */
int dadd_optim_adamw_step(float* p, float* g, float* m, float* v, float* ema, void* p16, long long n,
                          const int* group_chunks, int n_groups, const dadd_optim_state* state, float ema_weight,
                          int flags, int max_blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DADD_HIP_OPTIM_H */
