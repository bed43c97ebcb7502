// rip_fit.hip -- the resize stage on a window of F, and the letterbox bands (rip_set_output_roi / rip_set_output_fit, rip_fit.hpp;
// PARITY.md "Resize: window and fit").  Built into librip_fit_hip.so.
//
// The three window kernels are the bodies of rip_resize_dev.hpp with the window switch on -- linear_rows<CH, true>,
// mean2_rows<CH, true>, area_rows<CH, WHOLE, true> -- so their arithmetic is that of rip_resize.hip and rip_area.hip by
// construction: same tables, built for the window's size, same statements, same lane and workgroup geometry.  They differ in
// where they read (the header says how); the 2 x 2 mean shifts the dwords it has loaded by the phase of the window's first byte.
//
// fit_pad_kernel writes the pad colour to every pixel of F' outside the picture: a lane owns 4 consecutive pixels of a row, whole
// dwords where the row start is 4-byte aligned and all 4 are pad, single bytes otherwise.  Lanes inside the picture leave at once.
// Nothing is written at or beyond column `cols` of any row by any kernel here.
#include <hip/hip_runtime.h>

#include "rip_fit.hpp"
#include "rip_resize_dev.hpp"

namespace rip {
namespace {
template <int CH>
__global__ __launch_bounds__(kRszBlock) void fit_linear_kernel(ResizeParams p, FitWindow w) {
  linear_rows<CH, true>(p, w);
}

template <int CH>
__global__ __launch_bounds__(kRszBlock) void fit_mean2_kernel(ResizeParams p, FitWindow w) {
  mean2_rows<CH, true>(p, w);
}

template <int CH, bool WHOLE>
__global__ __launch_bounds__(kAreaBlock) void fit_area_kernel(AreaParams p, FitWindow w) {
  area_rows<CH, WHOLE, true>(p, w);
}

template <int CH>
__global__ __launch_bounds__(kRszBlock) void fit_pad_kernel(FitPadParams p) {
  const int x0 = ((int)blockIdx.x * kRszBlock + (int)threadIdx.x) * kRszPxPerLane;
  if (x0 >= p.cols) return;
  const int n = min(kRszPxPerLane, p.cols - x0);
  const int px1 = p.pic_x + p.pic_w, py1 = p.pic_y + p.pic_h;
  const bool in_cols = x0 >= p.pic_x && x0 + n <= px1;     // every pixel of the lane lies in the picture's columns
  const bool out_cols = x0 + n <= p.pic_x || x0 >= px1;    // none does
  uint8_t* dst_frame = p.dst + (size_t)blockIdx.z * p.dst_frame_stride;
  uint8_t v[4 * CH];
#pragma unroll
  for (int i = 0; i < 4 * CH; i++) v[i] = p.color[i % CH];
  for (int y = blockIdx.y; y < p.rows; y += gridDim.y) {
    const bool in_rows = y >= p.pic_y && y < py1;
    if (in_rows && in_cols) continue;
    uint8_t* row = dst_frame + (size_t)y * p.dst_step;
    uint8_t* q = row + (size_t)x0 * CH;
    if (!in_rows || out_cols) {
      store_pixels<CH>(q, v, n, (reinterpret_cast<uintptr_t>(row) & 3) == 0);
    } else {  // the lane straddles an edge of the picture: the pixels outside it, byte by byte
#pragma unroll
      for (int j = 0; j < kRszPxPerLane; j++)
        if (j < n && (x0 + j < p.pic_x || x0 + j >= px1)) {
#pragma unroll
          for (int c = 0; c < CH; c++) q[j * CH + c] = v[c];
        }
    }
  }
}
}  // namespace

bool launch_fit_resize(const ResizeParams& p, const FitWindow& w, hipStream_t stream, LaunchInfo* info) {
  bool mean2;
  if (!layout_ok(p, w) || !linear_ok(p, &mean2)) return false;
  static const NamedKernel<ResizeParams, FitWindow> kernels[2][2] = {{RIP_NAMED_KERNEL(fit_linear_kernel<1>), RIP_NAMED_KERNEL(fit_mean2_kernel<1>)},
                                                                     {RIP_NAMED_KERNEL(fit_linear_kernel<3>), RIP_NAMED_KERNEL(fit_mean2_kernel<3>)}};
  launch_variant(kernels, p.channels, mean2, rsz_grid(p.rows, p.cols, p.n_frames), kRszBlock, stream, info, p, w);
  return true;
}

bool launch_fit_area(const AreaParams& p, const FitWindow& w, hipStream_t stream, LaunchInfo* info) {
  bool whole;
  if (!layout_ok(p, w) || !area_ok(p, &whole)) return false;
  static const NamedKernel<AreaParams, FitWindow> kernels[2][2] = {{RIP_NAMED_KERNEL(fit_area_kernel<1, false>), RIP_NAMED_KERNEL(fit_area_kernel<1, true>)},
                                                                   {RIP_NAMED_KERNEL(fit_area_kernel<3, false>), RIP_NAMED_KERNEL(fit_area_kernel<3, true>)}};
  launch_variant(kernels, p.channels, whole, area_grid(p.rows, p.cols, p.n_frames), kAreaBlock, stream, info, p, w);
  return true;
}

bool launch_fit_pad(const FitPadParams& p, hipStream_t stream, LaunchInfo* info) {
  if (!p.dst || p.n_frames < 1 || p.n_frames > 65535 || (p.channels != 1 && p.channels != 3)) return false;
  if (p.rows < 1 || p.cols < 1 || p.rows > kRszMaxSide || p.cols > kRszMaxSide) return false;
  if (p.pic_w < 1 || p.pic_h < 1 || p.pic_x < 0 || p.pic_y < 0 || p.pic_x > p.cols - p.pic_w || p.pic_y > p.rows - p.pic_h) return false;
  if (p.pic_w == p.cols && p.pic_h == p.rows) return false;  // no band
  if (p.dst_step < (size_t)p.cols * p.channels) return false;
  const dim3 grid = rsz_grid(p.rows, p.cols, p.n_frames);
  if (p.channels == 1) hipLaunchKernelGGL((fit_pad_kernel<1>), grid, dim3(kRszBlock), 0, stream, p);
  else hipLaunchKernelGGL((fit_pad_kernel<3>), grid, dim3(kRszBlock), 0, stream, p);
  if (info) *info = LaunchInfo{p.channels == 1 ? "fit_pad_kernel<1>" : "fit_pad_kernel<3>", grid.x, grid.y, (unsigned)kRszBlock};
  return true;
}

}  // namespace rip
