// rip_area.hpp -- the resize stage under rip_set_output_interpolation("area"): cv::resize(F, size, INTER_AREA) for downscales of the
// pipeline's final 8-bit image (PARITY.md "Resize: area interpolation").  The kernels live in a library of their own,
// librip_area_hip.so (rip_area.hip): this header is its whole interface -- plain data and one launch function, which rip_batch.cpp
// calls.  The tables are built on the host (rip::build_resize_area_tables, rip_host.hpp).  Identity sizes launch nothing and the
// exact 2 x 2 case is the mean kernel of rip_resize.hpp: neither comes here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rip_launch_info.hpp"
#include "rip_resize.hpp"

namespace rip {

// Geometry of the kernel: a workgroup of kAreaBlock lanes (kAreaWaves waves) owns a rectangle of kAreaTileCols x kAreaTileRows
// output pixels of one frame; a lane owns one output column of it, wave w the rows w, w + kAreaWaves, ... of the rectangle.
// grid = (ceil(cols / kAreaTileCols), ceil(rows / kAreaTileRows), frames).
constexpr int kAreaBlock = 256;
constexpr int kAreaTileCols = 64;
constexpr int kAreaWaves = kAreaBlock / kAreaTileCols;
constexpr int kAreaTileRows = 8;
constexpr int kAreaMaxSide = 16384;   // of the source and of the target
constexpr int kAreaMaxFactor = 256;   // source side <= kAreaMaxFactor * target side: a block sum stays below 2^24

struct AreaParams {
  // F: interleaved uint8, 1 or 3 channels.  src, src_step and src_frame_stride are multiples of 4 and every dword that holds a byte
  // of a row lies inside the row's src_step bytes (the kernel reads whole dwords: the last one of a row may reach into the pitch)
  const uint8_t* src;
  size_t src_step, src_frame_stride;
  // F': the caller's buffer or the converter's staging image; any alignment.  Nothing is written at or beyond column `cols`.
  uint8_t* dst;
  size_t dst_step, dst_frame_stride;
  int src_rows, src_cols, rows, cols;  // R x C of F, H x W of F'; each in 1 .. kAreaMaxSide, H <= R <= 256 H, W <= C <= 256 W
  int channels, n_frames;
  // whole != 0: R % H == 0 and C % W == 0; every output pixel is the sum of its ky x kx block times `scale` = 1.f / (ky * kx); no
  // table is read
  int whole;
  float scale;
  // whole == 0: the per-axis tap lists on the device (build_resize_area_tables), 4-byte aligned.  Output column x reads the
  // xcount[x] consecutive source columns from xfirst[x] on with the weights xweight[xwofs[x] ...]; rows alike.
  const int32_t *xfirst, *xcount, *xwofs;
  const float* xweight;
  const int32_t *yfirst, *ycount, *ywofs;
  const float* yweight;
};

// Enqueues one area resize of n_frames frames on `stream`.  false -- nothing launched -- for sizes or channel counts outside the
// limits, an upscale on either axis, the identity, pitches that break the alignment rules above, a `whole` flag that does not match
// the sizes, or a missing table.
__attribute__((visibility("default"))) bool launch_area_reduce(const AreaParams& p, hipStream_t stream, LaunchInfo* info);

}  // namespace rip
