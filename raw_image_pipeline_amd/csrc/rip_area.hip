// rip_area.hip -- the resize stage under "area" interpolation (rip_set_output_interpolation, rip_area.hpp): cv::resize(F, size,
// INTER_AREA) for downscales of the pipeline's final 8-bit image of 1 or 3 interleaved channels, one launch per batch slice.  Built
// into librip_area_hip.so.
//
// The arithmetic, the geometry and the traffic are area_rows<CH, WHOLE, false> of rip_resize_dev.hpp, reading all of F (PARITY.md
// "Resize: area interpolation").  This file holds the kernel's entry point and its launch.
//
// Source rows are 4-byte aligned (rip_area.hpp).  The destination is the caller's, at any alignment.  Nothing is written at or
// beyond column `cols` of any row.
#include <hip/hip_runtime.h>

#include "rip_resize_dev.hpp"

namespace rip {
namespace {
template <int CH, bool WHOLE>
__global__ __launch_bounds__(kAreaBlock) void area_reduce_kernel(AreaParams p) {
  area_rows<CH, WHOLE, false>(p, FitWindow{});
}
}  // namespace

bool launch_area_reduce(const AreaParams& p, hipStream_t stream, LaunchInfo* info) {
  bool whole;
  if (!layout_ok(p, whole_frame(p.src_rows, p.src_cols)) || !area_ok(p, &whole)) return false;
  static const NamedKernel<AreaParams> kernels[2][2] = {{RIP_NAMED_KERNEL(area_reduce_kernel<1, false>), RIP_NAMED_KERNEL(area_reduce_kernel<1, true>)},
                                                        {RIP_NAMED_KERNEL(area_reduce_kernel<3, false>), RIP_NAMED_KERNEL(area_reduce_kernel<3, true>)}};
  launch_variant(kernels, p.channels, whole, area_grid(p.rows, p.cols, p.n_frames), kAreaBlock, stream, info, p);
  return true;
}

}  // namespace rip
