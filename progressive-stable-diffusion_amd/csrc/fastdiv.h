// Exact unsigned division by a run-time divisor without the ~35-instruction VALU sequence of a 32-bit division: the
// launcher computes a multiplier per divisor once (dadd_igemm_resolve), the kernels multiply and shift.
//
//   l = ceil(log2 d),  mul = ceil(2^(24 + l) / d),  n / d = (n * mul) >> (24 + l)      for every 0 <= n < 2^24
//
// (Granlund & Montgomery, "Division by invariant integers using multiplication", 1994: mul * d - 2^(24+l) < 2^l, so the
// error of n * mul / 2^(24+l) against n / d stays below 1 / d for n < 2^24.)  mul <= 2^25 fits 32 bits; with the dividend
// shifted left by 8 the product's upper word is (n * mul) >> 24: one v_lshlrev, one v_mul_hi_u32, one v_lshrrev.
// Plain C++: the host test (tests/test_fastdiv_cpu.py) compiles this header without a GPU compiler.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DADD_FASTDIV_HD __host__ __device__
#else
#define DADD_FASTDIV_HD
#endif

constexpr uint32_t DADD_FASTDIV_MAX = 1u << 24;   // dividends below, divisors up to this value

struct dadd_fastdiv {
  uint32_t mul, shift;
};

// 1 <= d <= 2^24 (host side)
static inline dadd_fastdiv dadd_fastdiv_make(uint32_t d) {
  uint32_t l = 0;
  while ((1u << l) < d) ++l;
  const uint64_t p = 1ull << (24 + l);
  return dadd_fastdiv{(uint32_t)((p + d - 1) / d), l};
}

// n / d for n < 2^24
DADD_FASTDIV_HD static inline uint32_t dadd_fastdiv_div(uint32_t n, dadd_fastdiv f) {
  return (uint32_t)(((uint64_t)(n << 8) * f.mul) >> 32) >> f.shift;
}
