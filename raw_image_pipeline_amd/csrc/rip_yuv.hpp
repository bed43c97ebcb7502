// rip_yuv.hpp -- the YUV 4:2:0 output formats (rip_set_output_format "nv12" / "i420", rip_set_output_yuv_matrix): one exact integer
// conversion of the delivered 8-bit BGR picture into a Y plane and subsampled Cb / Cr (PARITY.md "Output formats: YUV 4:2:0").  The
// kernel lives in a library of its own, librip_yuv_hip.so (rip_yuv.hip): this header is its whole interface -- plain data and one
// launch function, which rip_batch.cpp calls where it calls launch_output_convert for the other formats.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rip_launch_info.hpp"

namespace rip {

// Geometry of the kernel: every lane owns 2 rows x kYuvPxPerLane columns (four 2 x 2 blocks); a workgroup of kYuvBlock lanes is
// kYuvLanesX lanes wide -- kYuvPxPerBlockX columns -- and kYuvPairsPerBlock row pairs high;
// grid = (ceil(cols / kYuvPxPerBlockX), min(ceil(rows / 2 / kYuvPairsPerBlock), 65535), frames), row pairs strided over grid.y.
constexpr int kYuvBlock = 256;
constexpr int kYuvLanesX = 64;
constexpr int kYuvPxPerLane = 8;
constexpr int kYuvPxPerBlockX = kYuvLanesX * kYuvPxPerLane;
constexpr int kYuvPairsPerBlock = kYuvBlock / kYuvLanesX;

// One row of the table of matrices: Y = (yb B + yg G + yr R + (yoff << 15) + 16384) >> 15 per pixel; per 2 x 2 block with the channel
// sums SB, SG, SR: Cb = min(255, (cbb SB + cbg SG + cbr SR + (128 << 17) + 65536) >> 17), Cr alike.
struct YuvMatrix {
  int y[3], cb[3], cr[3];  // the weights of B, G, R
  int yoff;
};

struct Yuv420Params {
  // the delivered picture: interleaved BGR of uint8, rows x cols with both even.  src, src_step and src_frame_stride are multiples of 4
  // and a row's src_step bytes are readable (the kernel reads whole dwords: the last one of a row may reach into the pitch)
  const uint8_t* src;
  size_t src_step, src_frame_stride;
  // the caller's destination, any byte alignment: rows of dst_step bytes.  Y row y at y * dst_step.  Semi-planar (nv12): chroma row j
  // at (rows + j) * dst_step, bytes Cb Cr Cb Cr ...  Planar (i420; dst_step even): Cb row j at rows * dst_step + j * (dst_step / 2),
  // Cr row j (rows / 2) * (dst_step / 2) behind it.  Only cols bytes of a Y or nv12 chroma row and cols / 2 of an i420 chroma row are written.
  uint8_t* dst;
  size_t dst_step, dst_frame_stride;
  int rows, cols, n_frames;
  int semi_planar;  // 1: nv12, 0: i420
  YuvMatrix m;
};

// Enqueues one conversion of n_frames frames on `stream`.  false -- nothing launched -- for an empty or odd-sized picture, source
// pitches that break the alignment rule above, a destination pitch below a row or an odd one under i420.
__attribute__((visibility("default"))) bool launch_yuv420(const Yuv420Params& p, hipStream_t stream, LaunchInfo* info);

}  // namespace rip
