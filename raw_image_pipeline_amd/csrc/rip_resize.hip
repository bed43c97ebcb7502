// rip_resize.hip -- the resize stage (rip_set_output_size, rip_resize.hpp): cv::resize(F, size, INTER_LINEAR) on the pipeline's final
// 8-bit image of 1 or 3 interleaved channels, one launch per batch slice.  Built into librip_rsz_hip.so.
//
// The arithmetic is rip_resize_dev.hpp's, reading all of F: linear_rows<CH, false> and, when the source is exactly twice the target
// on both axes, mean2_rows<CH, false> (PARITY.md "Resize").  This file holds the two kernels' entry points and their launch.
//
// Source rows are 4-byte aligned.  The destination is the caller's: dword stores only where the row start is 4-byte aligned (the
// lanes of a row start whole stores apart, so the test is per row and wave-uniform), single bytes otherwise and for the 1 - 3
// pixels at a row's end.  Nothing is written at or beyond column `cols` of any row.
#include <hip/hip_runtime.h>

#include "rip_resize_dev.hpp"

namespace rip {
namespace {
template <int CH, bool AREA>
__global__ __launch_bounds__(kRszBlock) void resize_kernel(ResizeParams p) {
  if constexpr (AREA) mean2_rows<CH, false>(p, FitWindow{});
  else linear_rows<CH, false>(p, FitWindow{});
}
}  // namespace

bool launch_resize(const ResizeParams& p, hipStream_t stream, LaunchInfo* info) {
  bool mean2;
  if (!layout_ok(p, whole_frame(p.src_rows, p.src_cols)) || !linear_ok(p, &mean2)) return false;
  static const NamedKernel<ResizeParams> kernels[2][2] = {{RIP_NAMED_KERNEL(resize_kernel<1, false>), RIP_NAMED_KERNEL(resize_kernel<1, true>)},
                                                          {RIP_NAMED_KERNEL(resize_kernel<3, false>), RIP_NAMED_KERNEL(resize_kernel<3, true>)}};
  launch_variant(kernels, p.channels, mean2, rsz_grid(p.rows, p.cols, p.n_frames), kRszBlock, stream, info, p);
  return true;
}

}  // namespace rip
