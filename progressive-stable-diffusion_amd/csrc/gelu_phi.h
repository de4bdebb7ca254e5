// The normal CDF and density behind the derivative of the exact-form GELU, shared by geglu_grad (norm_grad.hip) and
// gelu_grad (cond_grad.hip).
#pragma once
#include "dadd_common.h"

// gelu and its derivative share the erf of dadd_gelu (Abramowitz & Stegun 7.1.26):
// Phi(g) = (1 + erf(g/sqrt2))/2 and phi(g) = exp(-g^2/2)/sqrt(2 pi), the exponential being the one inside the erf.
// gelu'(g) = Phi(g) + g phi(g).
__device__ __forceinline__ void dadd_gelu_phi(float g, float& Phi, float& phi) {
  const float z = fabsf(g) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  const float e = __builtin_amdgcn_exp2f(-z * z * 1.4426950408889634f);
  const float erf_abs = fmaf(-p * t, e, 1.0f);
  Phi = 0.5f * (1.0f + copysignf(erf_abs, g));
  phi = 0.39894228040143267794f * e;
}
