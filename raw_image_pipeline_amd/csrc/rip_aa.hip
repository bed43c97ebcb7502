// rip_aa.hip -- the resize stage under the antialiased filters "linear_aa" and "cubic_aa" (rip_set_output_interpolation,
// rip_aa.hpp): torch's F.interpolate(uint8, antialias=True) for downscales and upscales of the pipeline's final 8-bit image of 1 or 3
// interleaved channels, one launch per batch slice.  Built into librip_aa_hip.so.
//
// The arithmetic, the geometry and the traffic are aa_phase1 / aa_phase2 of rip_aa_dev.hpp (PARITY.md "Resize: antialiased
// filters"): the uint8 image between the horizontal and the vertical pass lives in the workgroup's LDS, whose size is a launch
// parameter.  This file holds the kernel's entry point and its launch.  aa_kernel<CH, false> reads all of F, aa_kernel<CH, true> a
// window of F in place.
//
// Source rows are 4-byte aligned (rip_aa.hpp).  The destination is the caller's, at any alignment.  Nothing is written at or beyond
// column `cols` of any row.
#include <hip/hip_runtime.h>

#include "rip_aa_dev.hpp"

namespace rip {
namespace {
template <int CH, bool WIN>
__global__ __launch_bounds__(kAaBlock) void aa_kernel(AaParams p, FitWindow w) {
  HIP_DYNAMIC_SHARED(uint8_t, aa_lds)
  aa_phase1<CH, WIN>(p, w, aa_lds);
  __syncthreads();
  aa_phase2<CH, WIN>(p, w, aa_lds);
}
}  // namespace

bool launch_aa(const AaParams& p, const FitWindow& w, hipStream_t stream, LaunchInfo* info) {
  if (!layout_ok(p, w) || !aa_ok(p)) return false;
  const bool win = w.x != 0 || w.y != 0 || w.frame_cols != p.src_cols || w.frame_rows != p.src_rows;
  static const NamedKernel<AaParams, FitWindow> kernels[2][2] = {{RIP_NAMED_KERNEL(aa_kernel<1, false>), RIP_NAMED_KERNEL(aa_kernel<1, true>)},
                                                                 {RIP_NAMED_KERNEL(aa_kernel<3, false>), RIP_NAMED_KERNEL(aa_kernel<3, true>)}};
  const NamedKernel<AaParams, FitWindow>& k = kernels[p.channels == 3][win];
  const dim3 grid = aa_grid(p);
  const size_t lds_bytes = (size_t)p.lds_rows * kAaTileCols * p.channels;
  hipLaunchKernelGGL(k.fn, grid, dim3(kAaBlock), lds_bytes, stream, p, w);
  if (info) *info = LaunchInfo{k.name, grid.x, grid.y, (unsigned)kAaBlock};
  return true;
}

}  // namespace rip
