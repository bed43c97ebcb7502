// rip_jpeg.hip -- the JPEG output format (rip_set_output_format "jpeg", rip_jpeg.hpp): the delivered picture -> one baseline JFIF
// stream per frame, in four launches per batch slice.  Built into librip_jpeg_hip.so.  The device code is rip_jpeg_dev.hpp.
//
// Nothing is written before a frame's length is known: the sizing pass counts, the scan decides, and the writing pass stores every
// interval at its final position inside the caller's slot -- or leaves the slot alone where the stream does not fit.  The scratch is
// the quantised coefficients (2 bytes per coded sample) and one word per restart interval; no stream is ever staged.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rip_jpeg_dev.hpp"

namespace rip {
namespace {

template <bool Colour>
__global__ __launch_bounds__(kJpegBlock) void jpeg_transform_kernel(JpegParams p) {
  jpeg_transform<Colour>(p);
}
__global__ __launch_bounds__(kJpegBlock) void jpeg_size_kernel(JpegParams p) { jpeg_size(p); }
__global__ __launch_bounds__(kJpegBlock) void jpeg_scan_kernel(JpegParams p) { jpeg_scan(p); }
__global__ __launch_bounds__(kJpegBlock) void jpeg_write_kernel(JpegParams p) { jpeg_write(p); }

unsigned groups(size_t items) { return (unsigned)((items + kJpegBlock - 1) / kJpegBlock); }

}  // namespace

bool launch_jpeg_transform(const JpegParams& p, hipStream_t stream, LaunchInfo* info) {
  if (!jpeg_ok(p)) return false;
  const dim3 grid(groups(jpeg_blocks(p.rows, p.cols, p.channels)), 1, (unsigned)p.n_frames);
  if (p.channels == 3) hipLaunchKernelGGL(jpeg_transform_kernel<true>, grid, dim3(kJpegBlock), 0, stream, p);
  else hipLaunchKernelGGL(jpeg_transform_kernel<false>, grid, dim3(kJpegBlock), 0, stream, p);
  if (info) *info = LaunchInfo{p.channels == 3 ? "jpeg_transform_kernel<true>" : "jpeg_transform_kernel<false>", grid.x, grid.y, (unsigned)kJpegBlock};
  return true;
}

bool launch_jpeg_size(const JpegParams& p, hipStream_t stream, LaunchInfo* info) {
  if (!jpeg_ok(p)) return false;
  const dim3 grid(groups((size_t)jpeg_intervals(p.rows, p.channels, p.restart_rows)), 1, (unsigned)p.n_frames);
  hipLaunchKernelGGL(jpeg_size_kernel, grid, dim3(kJpegBlock), 0, stream, p);
  if (info) *info = LaunchInfo{"jpeg_size_kernel", grid.x, grid.y, (unsigned)kJpegBlock};
  return true;
}

bool launch_jpeg_scan(const JpegParams& p, hipStream_t stream, LaunchInfo* info) {
  if (!jpeg_ok(p)) return false;
  const dim3 grid(groups((size_t)p.n_frames), 1, 1);
  hipLaunchKernelGGL(jpeg_scan_kernel, grid, dim3(kJpegBlock), 0, stream, p);
  if (info) *info = LaunchInfo{"jpeg_scan_kernel", grid.x, grid.y, (unsigned)kJpegBlock};
  return true;
}

bool launch_jpeg_write(const JpegParams& p, hipStream_t stream, LaunchInfo* info) {
  if (!jpeg_ok(p)) return false;
  const dim3 grid(groups((size_t)jpeg_intervals(p.rows, p.channels, p.restart_rows)) + 1, 1, (unsigned)p.n_frames);
  hipLaunchKernelGGL(jpeg_write_kernel, grid, dim3(kJpegBlock), 0, stream, p);
  if (info) *info = LaunchInfo{"jpeg_write_kernel", grid.x, grid.y, (unsigned)kJpegBlock};
  return true;
}

}  // namespace rip
