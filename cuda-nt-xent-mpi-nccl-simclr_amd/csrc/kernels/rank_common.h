// What the two rank kernel files (rank_kernels.hip, xview_rank_kernels.hip) share: the
// order-preserving integer image of a float, for integer atomic maxima, and the integer DPP row sum
// of their byte-packed counts. Device code only.
#pragma once
#include "device_common.h"

namespace ntxent {
namespace dev {

// Order-preserving integer image of a float (signed compare): negative floats are mirrored.
__device__ __forceinline__ int f2ord(float x) {
  const int b = __float_as_int(x);
  return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float ord2f(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

template <int CTRL> __device__ __forceinline__ int dpp_i(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true);
}
// sum over the 16 lanes of a DPP row (every lane gets it)
__device__ __forceinline__ int row16_isum(int x) {
  x += dpp_i<0x128>(x);
  x += dpp_i<0x124>(x);
  x += dpp_i<0x122>(x);
  x += dpp_i<0x121>(x);
  return x;
}

}  // namespace dev
}  // namespace ntxent
