"""CPU: the multiply-shift division of csrc/fastdiv.h against `/` and `%`.

A stand-alone host program (own main) includes the header and checks, for every divisor 1 .. 4096 and every Wo and
Ho * Wo with Ho, Wo <= 512, the dividends on both sides of every multiple of the divisor below 2^24 (k d - 1, k d,
k d + 1), the ends of the range, and all of [0, 2^24) for a few divisors; a quotient is wrong first at such a multiple.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "progressive-stable-diffusion_amd", "csrc")

PROGRAM = r"""
#include "fastdiv.h"
#include <cstdio>
#include <vector>

static unsigned long long checked = 0;
static int bad = 0;

static void check(uint32_t n, uint32_t d, dadd_fastdiv f) {
  const uint32_t q = dadd_fastdiv_div(n, f);
  ++checked;
  if (q != n / d || n - q * d != n % d) {
    if (bad < 10) std::printf("WRONG %u / %u: got %u, want %u\n", n, d, q, n / d);
    ++bad;
  }
}

int main() {
  const uint32_t LIM = DADD_FASTDIV_MAX;
  std::vector<char> want(512 * 512 + 1, 0);
  for (uint32_t d = 1; d <= 4096; ++d) want[d] = 1;
  for (uint32_t h = 1; h <= 512; ++h)
    for (uint32_t w = 1; w <= 512; ++w) want[h * w] = 1;
  unsigned divisors = 0;
  for (uint32_t d = 1; d <= 512 * 512; ++d) {
    if (!want[d]) continue;
    ++divisors;
    const dadd_fastdiv f = dadd_fastdiv_make(d);
    check(0, d, f);
    check(LIM - 1, d, f);
    for (uint64_t m = d; m < LIM; m += d) {
      check((uint32_t)m - 1, d, f);
      check((uint32_t)m, d, f);
      if (m + 1 < LIM) check((uint32_t)m + 1, d, f);
    }
  }
  const uint32_t full[] = {1, 2, 3, 7, 9, 144, 320, 1024, 4095, 4096, 36864, 262144, 1u << 24};
  for (uint32_t d : full) {
    const dadd_fastdiv f = dadd_fastdiv_make(d);
    for (uint32_t n = 0; n < LIM; ++n) check(n, d, f);
  }
  std::printf("divisors %u checked %llu bad %d\n", divisors, checked, bad);
  return bad ? 1 : 0;
}
"""


def test_fastdiv_matches_division(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if cxx is None and not os.path.exists(hipcc):
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "fastdiv_check.cpp", tmp_path / "fastdiv_check"
    src.write_text(PROGRAM)
    cmd = [cxx, "-O2", "-std=c++17"] if cxx else [hipcc, "-O2", "-std=c++17", "-x", "c++"]
    subprocess.run(cmd + ["-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " bad 0" in r.stdout, r.stdout
