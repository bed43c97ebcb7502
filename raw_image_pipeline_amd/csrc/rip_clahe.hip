// rip_clahe.hip -- contrast-limited adaptive histogram equalisation of a delivered one-channel picture (rip_set_output_clahe,
// rip_clahe.hpp): cv::CLAHE for CV_8UC1 restated (PARITY.md "Local contrast: CLAHE"), two launches per batch slice at the end of a
// head's launches.  Built into librip_clahe_hip.so.
//
// The arithmetic, the geometry and the traffic are the phase functions of rip_clahe_dev.hpp; this file holds the kernels' entry
// points -- the phases around their barriers -- and the launches.  clahe_lut_kernel reads the picture once, 1 B/px, and writes 256
// bytes per (tile, frame); clahe_apply_kernel reads and writes the picture, 1 + 1 B/px, and is expected to be bound by its four LDS
// byte look-ups per pixel.
//
// Source and destination are the caller's at any alignment, or the staging image; the destination may be the source.  Nothing is
// written outside the picture's cols bytes of a row: pad bands, row padding and frame gaps keep their bytes.
#include <hip/hip_runtime.h>

#include "rip_clahe_dev.hpp"

namespace rip {
namespace {
__global__ __launch_bounds__(kClaheBlock) void clahe_lut_kernel(ClaheParams p) {
  HIP_DYNAMIC_SHARED(uint32_t, clahe_hist)
  clahe_lut_zero(p, clahe_hist);
  __syncthreads();
  clahe_lut_count(p, clahe_hist);
  __syncthreads();
  clahe_lut_clip(p, clahe_hist);
  __syncthreads();
  clahe_lut_spread(p, clahe_hist);
  __syncthreads();
  clahe_lut_store(p, clahe_hist);
}

__global__ __launch_bounds__(kClaheBlock) void clahe_apply_kernel(ClaheParams p, int strip_rows) {
  HIP_DYNAMIC_SHARED(uint8_t, clahe_tables)
  clahe_apply_stage(p, strip_rows, clahe_tables);
  __syncthreads();
  clahe_apply_blend(p, strip_rows, clahe_tables);
}
}  // namespace

bool launch_clahe_lut(const ClaheParams& p, hipStream_t stream, LaunchInfo* info) {
  if (!clahe_ok(p)) return false;
  const dim3 grid((unsigned)p.tiles_x, (unsigned)p.tiles_y, (unsigned)p.n_frames);
  hipLaunchKernelGGL(clahe_lut_kernel, grid, dim3(kClaheBlock), (size_t)kClaheLutLdsBytes, stream, p);
  if (info) *info = LaunchInfo{"clahe_lut_kernel", grid.x, grid.y, (unsigned)kClaheBlock};
  return true;
}

bool launch_clahe_apply(const ClaheParams& p, hipStream_t stream, LaunchInfo* info) {
  if (!clahe_ok(p)) return false;
  const int strip_rows = clahe_strip_rows(p);
  const dim3 grid(1u, (unsigned)((p.tiles_y + 1) * (p.th / strip_rows + 1)), (unsigned)p.n_frames);
  hipLaunchKernelGGL(clahe_apply_kernel, grid, dim3(kClaheBlock), (size_t)2 * p.tiles_x * kClaheBins, stream, p, strip_rows);
  if (info) *info = LaunchInfo{"clahe_apply_kernel", grid.x, grid.y, (unsigned)kClaheBlock};
  return true;
}

}  // namespace rip
