// rip_mask.hpp -- valid-pixel masks (rip_set_rect_mask; PARITY.md "Rect mask"): the coverage mask of an undistortion, which is
// cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) of an all-255 image computed from the maps alone, and the threshold that turns a
// coverage image into a valid mask.  The kernels live in a library of their own, librip_mask_hip.so (rip_mask.hip): this header is
// its whole interface -- plain data and two launch functions, which rip_batch.cpp calls.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rip_launch_info.hpp"

namespace rip {

// Geometry of both kernels (the converter's shape, rip_output.hpp): every lane owns kMaskPxPerLane consecutive pixels of one row, a
// workgroup of kMaskBlock lanes covers kMaskPxPerBlock pixels of one row; grid = (ceil(cols / kMaskPxPerBlock), min(rows, 65535))
// with a row loop.
constexpr int kMaskBlock = 256;
constexpr int kMaskPxPerLane = 4;
constexpr int kMaskPxPerBlock = kMaskBlock * kMaskPxPerLane;

struct RectMaskParams {
  // the undistortion maps as the handle keeps them on the device: interleaved (x, y) floats, drows x dcols entries, rows tight --
  // 8 bytes per entry, so a row starts 16-byte aligned only where y * dcols is even; map_xy itself is 8-byte aligned at least
  const float* map_xy;
  int drows, dcols;
  // the image that enters the remap (after the flip): only its size matters, no pixel of it is read
  int src_rows, src_cols;
  // the mask, one byte per map entry: any alignment, any pitch of at least dcols.  Nothing is written at or beyond dcols of a row.
  uint8_t* dst;
  size_t dst_step;
  int binary;  // 0: the coverage M (0..255); 1: (M == 255) ? 255 : 0
};

struct MaskThresholdParams {
  // an image of rows x cols bytes, thresholded in place: v = (v == 255) ? 255 : 0.  img and step are multiples of 4 and a row's
  // step bytes belong to the image (the kernel works on whole dwords: the last one of a row may reach into the pitch, never beyond it)
  uint8_t* img;
  size_t step;
  int rows, cols;
};

// Enqueue one launch on `stream`.  false -- nothing launched -- for a null pointer, an empty image or source, or pointers and
// pitches that break the rules above.
__attribute__((visibility("default"))) bool launch_rect_mask(const RectMaskParams& p, hipStream_t stream, LaunchInfo* info);
__attribute__((visibility("default"))) bool launch_mask_threshold(const MaskThresholdParams& p, hipStream_t stream, LaunchInfo* info);

}  // namespace rip
