// rip_heads.hpp -- output heads (rip_set_output_heads, rip_apply_device_heads): the copy that delivers the pipeline's final image F
// to a further head that asks for F as it is, out of the staging image the other heads read.  The kernel lives in a library of its
// own, librip_heads_hip.so (rip_heads.hip): this header is its whole interface -- plain data and one launch function, which
// rip_batch.cpp calls.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rip_launch_info.hpp"

namespace rip {

// Geometry of the kernel (the converter's shape, rip_output.hpp): every lane owns kHeadBytesPerLane consecutive source bytes of one
// row, a workgroup of kHeadBlock lanes covers kHeadBytesPerBlock bytes of one row; grid = (ceil(row_bytes / kHeadBytesPerBlock),
// min(rows, 65535), frames) with a row loop.
constexpr int kHeadBlock = 256;
constexpr int kHeadBytesPerLane = 16;
constexpr int kHeadBytesPerBlock = kHeadBlock * kHeadBytesPerLane;

struct HeadCopyParams {
  // the staging image: src, src_step and src_frame_stride are multiples of 16 and src_step holds row_bytes rounded up to 16 (the
  // kernel reads whole 16-byte blocks: the last one of a row may reach into the pitch, never beyond it)
  const uint8_t* src;
  size_t src_step, src_frame_stride;
  // the caller's buffer: any alignment, any pitch of at least row_bytes.  Nothing is written at or beyond row_bytes of a row.
  uint8_t* dst;
  size_t dst_step, dst_frame_stride;
  int rows, n_frames;
  size_t row_bytes;  // cols * channels, below 16 MiB
};

// Enqueues one copy of n_frames frames on `stream`.  false -- nothing launched -- for an empty image, more than 65535 frames or
// pitches that break the rules above.
__attribute__((visibility("default"))) bool launch_head_copy(const HeadCopyParams& p, hipStream_t stream, LaunchInfo* info);

}  // namespace rip
