// rip_resize.hpp -- the resize stage (rip_set_output_size): cv::resize(F, size, INTER_LINEAR) on the pipeline's final 8-bit image,
// between the last kernel of the chain and the output converter.  The kernels live in a library of their own,
// librip_rsz_hip.so (rip_resize.hip): this header is its whole interface -- plain data and one launch function, which
// rip_batch.cpp calls.  The tables are built on the host (rip::build_resize_tables, rip_host.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rip_launch_info.hpp"

namespace rip {

// Geometry of the kernel (the converter's, rip_output.hpp): every lane owns kRszPxPerLane consecutive output pixels of one row, a
// workgroup of kRszBlock lanes covers kRszPxPerBlock pixels of one row; grid = (ceil(cols / kRszPxPerBlock), min(rows, 65535), frames).
constexpr int kRszBlock = 256;
constexpr int kRszPxPerLane = 4;
constexpr int kRszPxPerBlock = kRszBlock * kRszPxPerLane;
constexpr int kRszMaxSide = 16384;  // of the source and of the target

// entries of the per-column tables on the device: cols rounded up to whole lanes (the padding is never used, only loaded)
inline size_t resize_table_cols(int cols) { return ((size_t)cols + kRszPxPerLane - 1) & ~(size_t)(kRszPxPerLane - 1); }

struct ResizeParams {
  // F: interleaved uint8, 1 or 3 channels.  src, src_step and src_frame_stride are multiples of 4 and every dword that holds a byte
  // of a row lies inside the row's src_step bytes (the kernel reads whole dwords: the last one of a row may reach into the pitch)
  const uint8_t* src;
  size_t src_step, src_frame_stride;
  // F': the caller's buffer or the converter's staging image; any alignment.  Nothing is written at or beyond column `cols`.
  uint8_t* dst;
  size_t dst_step, dst_frame_stride;
  int src_rows, src_cols, rows, cols;  // R x C of F, H x W of F'; each in 1 .. kRszMaxSide
  int channels, n_frames;
  int area2;  // R == 2 H and C == 2 W: the 2 x 2 mean, no table is read
  // tables on the device (build_resize_tables), all 16-byte aligned: xofs[resize_table_cols(W)], alpha[2 * resize_table_cols(W)]
  // (a0, a1 per column), yofs[2 * H] (the two clamped rows), beta[2 * H] (b0, b1 per row)
  const int32_t* xofs;
  const int16_t* alpha;
  const int32_t* yofs;
  const int16_t* beta;
};

// Where a window lies in F (rip_fit.hpp; the kernels of rip_resize_dev.hpp).  The params of a launch on a window describe the window
// as the whole-frame launches describe a frame -- src_rows x src_cols is the window's size and the tables are those of that size --
// while src, src_step and src_frame_stride stay those of F: pixel (u, v) of the window is pixel (x + u, y + v) of F.  frame_cols is
// C of F: the last dword of a row of F that may be read is the one that holds its last byte.
struct FitWindow {
  int x, y;        // >= 0
  int frame_cols;  // x + src_cols <= frame_cols
  int frame_rows;  // y + src_rows <= frame_rows
};

// Enqueues one resize of n_frames frames on `stream`.  false -- nothing launched -- for sizes or channel counts outside the limits,
// pitches that break the alignment rules above, or an area2 flag that does not match the sizes.
__attribute__((visibility("default"))) bool launch_resize(const ResizeParams& p, hipStream_t stream, LaunchInfo* info);

}  // namespace rip
