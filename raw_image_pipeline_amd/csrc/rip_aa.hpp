// rip_aa.hpp -- the resize stage under rip_set_output_interpolation("linear_aa" / "cubic_aa"): the antialiased separable filters of
// torch.nn.functional.interpolate(uint8, mode='bilinear' | 'bicubic', antialias=True) on the pipeline's final 8-bit image (PARITY.md
// "Resize: antialiased filters").  The kernels live in a library of their own, librip_aa_hip.so (rip_aa.hip): this header is its
// whole interface -- plain data and one launch function, which rip_batch.cpp calls.  The tables are built on the host
// (rip::build_resize_aa_tables, rip_host.hpp).  The identity launches nothing, or is the linear tables' copy: it does not come here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rip_launch_info.hpp"
#include "rip_resize.hpp"

namespace rip {

// Geometry of the kernel: a workgroup of kAaBlock lanes (kAaWaves waves) owns a rectangle of kAaTileCols x tile_rows output pixels
// of one frame; a lane owns one output column of it.  Phase 1: the waves stride the source rows the rectangle's output rows read
// and every lane writes the horizontal pass of its column, rounded to uint8, to LDS; phase 2: the waves stride the rectangle's
// output rows and every lane walks its vertical taps down the LDS column.  grid = (ceil(cols / kAaTileCols), ceil(rows / tile_rows),
// frames).  The LDS image is [source row of the span][channel][kAaTileCols] bytes.
constexpr int kAaBlock = 256;
constexpr int kAaTileCols = 64;
constexpr int kAaWaves = kAaBlock / kAaTileCols;
constexpr int kAaMaxTileRows = 8;         // tile_rows is 8, 4, 2 or 1
constexpr int kAaMaxSide = 16384;         // of the source and of the target
constexpr int kAaMaxFactor = 64;          // source side <= kAaMaxFactor * target side: the span of one output row fits the LDS budget
constexpr size_t kAaMaxLdsBytes = 65536;  // of one workgroup
constexpr int kAaMaxPrec = 22;            // weights are round(w * 2^prec), prec <= 22

struct AaParams {
  // F: interleaved uint8, 1 or 3 channels.  src, src_step and src_frame_stride are multiples of 4 and every dword that holds a byte
  // of a row lies inside the row's src_step bytes (the kernel reads whole dwords: the last one of a row may reach into the pitch)
  const uint8_t* src;
  size_t src_step, src_frame_stride;
  // F': the caller's buffer or the converter's staging image; any alignment.  Nothing is written at or beyond column `cols`.
  uint8_t* dst;
  size_t dst_step, dst_frame_stride;
  int src_rows, src_cols, rows, cols;  // R x C of F (or of the window), H x W of F'; each in 1 .. kAaMaxSide, R <= 64 H, C <= 64 W
  int channels, n_frames;
  // the launch's tile height and its LDS rows: every rectangle's output rows read at most lds_rows consecutive source rows
  // (build_resize_aa_tables); lds_rows * kAaTileCols * channels <= kAaMaxLdsBytes
  int tile_rows, lds_rows;
  // weights are int16, round(w * 2^prec) per axis; a pass is clamp((2^(prec - 1) + sum of taps) >> prec, 0, 255)
  int xprec, yprec;
  // the per-axis tap lists on the device, 4-byte aligned (weights: 2-byte).  Output column x reads the xcount[x] consecutive source
  // columns from xfirst[x] on with the weights xweight[xwofs[x] ...]; rows alike.  An axis that keeps its size (C == W, R == H) is
  // skipped -- phase 1 copies, phase 2 copies -- and its tables are not read.
  const int32_t *xfirst, *xcount, *xwofs;
  const int16_t* xweight;
  const int32_t *yfirst, *ycount, *ywofs;
  const int16_t* yweight;
};

// Enqueues one antialiased resize of n_frames frames on `stream`: of all of F when `w` is the whole frame, else of the window `w` of
// F, read in place (rip_resize.hpp FitWindow).  false -- nothing launched -- for sizes or channel counts outside the limits, a factor
// above kAaMaxFactor on an axis, the identity, pitches that break the alignment rules above, a window that does not lie inside F, a
// tile height or an LDS size outside the limits, or a missing table.
__attribute__((visibility("default"))) bool launch_aa(const AaParams& p, const FitWindow& w, hipStream_t stream, LaunchInfo* info);

}  // namespace rip
