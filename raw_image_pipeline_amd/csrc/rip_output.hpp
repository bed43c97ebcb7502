// rip_output.hpp -- the output stage (rip_set_output_format): one exact per-pixel conversion of the pipeline's final 8-bit BGR
// image into the format the caller asked for.  The kernels live in a library of their own, librip_out_hip.so (rip_output.hip):
// this header is its whole interface -- plain data and one launch function, which rip_batch.cpp calls.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rip_launch_info.hpp"

namespace rip {

// ids of the format names of rip.h, in the order rip_host.cpp kOutputFormatNames lists them
enum OutputFormat : int {
  OUT_NATIVE = 0,
  OUT_RGB8 = 1,
  OUT_MONO8 = 2,
  OUT_RGB_CHW_F32 = 3,
  OUT_RGB_CHW_F16 = 4,
  OUT_RGB_CHW_BF16 = 5,
  OUT_BGR_CHW_F32 = 6,
  OUT_BGR_CHW_F16 = 7,
  OUT_BGR_CHW_BF16 = 8,
  // YUV 4:2:0 for encoders: converted by yuv420_kernel of librip_yuv_hip.so (rip_yuv.hpp), not by this library's converter
  OUT_NV12 = 9,
  OUT_I420 = 10,
  // a baseline JPEG stream per frame: encoded by the kernels of librip_jpeg_hip.so (rip_jpeg.hpp), in the converter's place too
  OUT_JPEG = 11,
  OUT_FORMAT_COUNT = 12
};
inline bool output_format_yuv(int f) { return f == OUT_NV12 || f == OUT_I420; }
inline bool output_format_jpeg(int f) { return f == OUT_JPEG; }
inline bool output_format_planar(int f) { return f >= OUT_RGB_CHW_F32 && f <= OUT_BGR_CHW_BF16; }
inline bool output_format_rgb_planes(int f) { return f >= OUT_RGB_CHW_F32 && f <= OUT_RGB_CHW_BF16; }
// bytes per delivered element and delivered channels (planes) of a non-native format
inline int output_format_elem_bytes(int f) {
  return (f == OUT_RGB_CHW_F32 || f == OUT_BGR_CHW_F32) ? 4 : (output_format_planar(f) ? 2 : 1);
}
inline int output_format_channels(int f) { return f == OUT_MONO8 || output_format_yuv(f) || output_format_jpeg(f) ? 1 : 3; }

// Geometry of the converter (rip_output.hip): every lane owns kOutPxPerLane consecutive pixels of one row, a workgroup of
// kOutBlock lanes covers kOutPxPerBlock pixels of one row; grid = (ceil(cols / kOutPxPerBlock), min(rows, 65535), frames).
constexpr int kOutBlock = 256;
constexpr int kOutPxPerLane = 4;
constexpr int kOutPxPerBlock = kOutBlock * kOutPxPerLane;

struct OutputConvertParams {
  // the pipeline's final image: interleaved BGR of uint8.  src, src_step and src_frame_stride are multiples of 4 and a row's
  // src_step bytes are readable (the kernel reads whole dwords: the last one of a row may reach into the pitch)
  const uint8_t* src;
  size_t src_step, src_frame_stride;
  // the caller's destination; pitches in BYTES.  Interleaved formats: rows of dst_step bytes.  Planar formats: plane c of a
  // frame starts at c * dst_step * rows, its rows are dst_step bytes apart; dst, dst_step and dst_frame_stride are multiples of
  // the element size.  Nothing is written beyond a row's cols elements.
  void* dst;
  size_t dst_step, dst_frame_stride;
  int rows, cols, n_frames;
  int format;         // OutputFormat, not OUT_NATIVE
  const void* table;  // planar formats: 3 x 256 elements on the device, plane-major (rip::build_output_table)
};

// Enqueues one conversion of n_frames frames on `stream`.  false -- nothing launched -- for an unknown format, an empty image
// or pitches that break the alignment rules above.
__attribute__((visibility("default"))) bool launch_output_convert(const OutputConvertParams& p, hipStream_t stream, LaunchInfo* info);

}  // namespace rip
