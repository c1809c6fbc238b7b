// Host-side helpers the kernel files' launchers share.
#pragma once
#include "../include/ntxent/ntxent.h"
#include "device_common.h"

#include <string>

namespace ntxent {

inline int roundup(int x, int m) { return (x + m - 1) / m * m; }

template <typename F>
void dispatch_comp(DType t, F&& f) {
  switch (t) {
    case DType::F32: f(float{}); break;
    case DType::F16: f(_Float16{}); break;
    case DType::BF16: f(__bf16{}); break;
    case DType::FP8: NTXENT_CHECK(false, "fp8 is a GEMM operand type only"); break;
  }
}

// GEMM operand types (fp8 included).
template <typename F>
void dispatch_gemm(DType t, F&& f) {
  if (t == DType::FP8) f(dev::fp8e4m3{});
  else dispatch_comp(t, f);
}

// launch_prep's unit rows as the 128 x 128 tile kernels (tile128.h) read them: rows ldb bytes
// apart, nk K-steps of 128 bytes each. How many rows a kernel reads, of how many ranks, and so what
// row padding and world it needs, is for its launcher to check.
struct UnitRows {
  const char* ptr;
  long long ldb;
  int nk;
};
inline UnitRows unit_rows(DType comp, const void* zq, const Geometry& g, const std::string& who) {
  NTXENT_CHECK(comp == DType::F32 || comp == DType::F16 || comp == DType::BF16, who + ": fp32 | fp16 | bf16 rows");
  const size_t es = dtype_size(comp), kbytes = (size_t)g.dim_k * es;
  NTXENT_CHECK(kbytes % kKStepBytes == 0 && g.dim_k <= g.ld_k && kbytes >= kKStepBytes,
               who + ": geometry does not pad K to 128 bytes");
  return {static_cast<const char*>(zq), (long long)g.ld_k * (long long)es, (int)(kbytes / kKStepBytes)};
}

}  // namespace ntxent
