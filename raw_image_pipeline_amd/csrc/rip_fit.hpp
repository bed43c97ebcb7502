// rip_fit.hpp -- the resize stage's window and fit modes (rip_set_output_roi, rip_set_output_fit, rip_set_output_pad; PARITY.md
// "Resize: window and fit"): the kernels that read a window of F in place of all of F, and the kernel that fills the bands a
// letterbox leaves around the picture.  They live in a library of their own, librip_fit_hip.so (rip_fit.hip): this header is its
// whole interface -- plain data and three launch functions, which rip_batch.cpp calls; the parameter structs of the two resizes
// and the window (FitWindow) are those of rip_resize.hpp / rip_area.hpp.  A resize that reads all of F goes to those two headers' launches, whatever rectangle of F' it writes: only a window other than F comes here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rip_area.hpp"
#include "rip_launch_info.hpp"
#include "rip_resize.hpp"

namespace rip {

// the bands of F' outside the picture: every pixel of the rows x cols image that is not in the pic_w x pic_h rectangle at
// (pic_x, pic_y) gets `color` (channels bytes, B G R or one grey byte).  Any destination alignment; nothing is written at or
// beyond column `cols`.
struct FitPadParams {
  uint8_t* dst;
  size_t dst_step, dst_frame_stride;
  int rows, cols;  // H x W of F', each in 1 .. kRszMaxSide
  int pic_x, pic_y, pic_w, pic_h;
  int channels, n_frames;
  uint8_t color[4];
};

// launch_resize's work (the two-tap tables, or the 2 x 2 mean when p.area2) on a window of F; the same refusals, on the window's
// size, plus a window that does not lie inside F.  The grid is launch_resize's.
__attribute__((visibility("default"))) bool launch_fit_resize(const ResizeParams& p, const FitWindow& w, hipStream_t stream, LaunchInfo* info);
// launch_area_reduce's work on a window of F, on the same terms
__attribute__((visibility("default"))) bool launch_fit_area(const AreaParams& p, const FitWindow& w, hipStream_t stream, LaunchInfo* info);
// false -- nothing launched -- also when the picture covers all of F' (there is no band) or does not lie inside it.
// grid = (ceil(cols / kRszPxPerBlock), min(rows, 65535), frames): a lane owns kRszPxPerLane consecutive pixels of a row.
__attribute__((visibility("default"))) bool launch_fit_pad(const FitPadParams& p, hipStream_t stream, LaunchInfo* info);

}  // namespace rip
