// rip_round_map.hpp -- cv::remap's map quantiser, the one definition shared by the remap kernels (rip_remap_dev.hpp) and the
// rect-mask kernel (rip_mask.hip): a coverage mask is only the remap of a white image if both round a map entry the same way.
// Nothing but the function: the includer brings <hip/hip_runtime.h> (or tests/cpp/hip_host_stub in its place).
#pragma once
#include <climits>

namespace rip {
namespace {

// cvRound(v * 32): the map entry in 1/32 pixel; INT_MIN for NaN, inf and values outside int32 (what cvRound's cvtss2si gives)
__device__ __forceinline__ int round_map(float v) {
  float s = v * 32.f;
  if (!(s > -2147483648.f && s < 2147483648.f)) return INT_MIN;  // cvRound of NaN/inf/out of range
  return (int)__builtin_rintf(s);
}

}  // namespace
}  // namespace rip
