// rip_aa_dev.hpp -- the device code of rip_aa.hip and the checks its launch function makes (PARITY.md "Resize: antialiased
// filters").  Included by rip_aa.hip alone; the row reader and the layout check are those of rip_resize_dev.hpp.
//
// A workgroup owns 64 output columns x p.tile_rows output rows of one frame, a lane one output column.  The two passes of the
// definition -- horizontal over every source row, rounded to uint8, then vertical over that -- meet in LDS: no intermediate image
// exists in global memory.
//   aa_phase1   the source rows [row_lo, row_hi) the rectangle's output rows read: wave w takes the rows row_lo + w, + 4, ...; a
//               lane walks its column's taps along the row (the read pattern of area_rows: aligned dwords, each loaded once per
//               row, none beyond the dword that holds the last byte of the row of F) and writes
//               clamp((2^(xprec - 1) + sum S[x_k] q_k) >> xprec, 0, 255) per channel to lds[(row - row_lo) * CH + c][lane]
//   barrier     every lane of the workgroup reaches it: a lane past `cols` does no work in either phase, and does not leave
//   aa_phase2   wave w takes the output rows y0 + w, + 4, ... of the rectangle; a lane walks its vertical taps down the LDS column
//               and stores clamp((2^(yprec - 1) + sum lds[y_j] q_j) >> yprec, 0, 255) as CH single bytes
// Integer work only: int32 sums, an arithmetic shift; no float, no division.  An axis that keeps its size is skipped: phase 1 copies
// the lane's pixel, phase 2 copies the LDS row.  With a factor of at most 64, 255 * sum |q| stays below 2^31.
//
// WIN: false reads all of F; true reads the window `w` of F in place, at any byte phase (rip_resize.hpp FitWindow).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "rip_aa.hpp"
#include "rip_resize_dev.hpp"

namespace rip {

// the rectangle's output rows [y0, y1] and the source rows [row_lo, row_hi) they read (the tap lists' first and first + count are
// non-decreasing along an axis)
struct AaSpan {
  int y0, y1, row_lo, row_hi;
};
__device__ __forceinline__ AaSpan aa_span(const AaParams& p) {
  AaSpan s;
  s.y0 = (int)blockIdx.y * p.tile_rows;
  s.y1 = min(p.rows, s.y0 + p.tile_rows) - 1;
  if (p.src_rows == p.rows) {
    s.row_lo = s.y0;
    s.row_hi = s.y1 + 1;
  } else {
    s.row_lo = p.yfirst[s.y0];
    s.row_hi = p.yfirst[s.y1] + p.ycount[s.y1];
  }
  return s;
}

__device__ __forceinline__ uint8_t aa_byte(int acc, int prec) { return (uint8_t)min(max(acc >> prec, 0), 255); }

template <int CH, bool WIN>
__device__ __forceinline__ void aa_phase1(const AaParams& p, const FitWindow& w, uint8_t* lds) {
  const int lane = (int)threadIdx.x % kAaTileCols, wave = (int)threadIdx.x / kAaTileCols;
  const int x = (int)blockIdx.x * kAaTileCols + lane;
  if (x >= p.cols) return;  // of the phase, not of the kernel
  const AaSpan s = aa_span(p);
  const int wx = WIN ? w.x : 0, frame_cols = WIN ? w.frame_cols : p.src_cols;
  const uint8_t* src_frame = p.src + (size_t)blockIdx.z * p.src_frame_stride;
  if constexpr (WIN) src_frame += (size_t)w.y * p.src_step;
  const int last_dw = ((frame_cols * CH + 3) >> 2) - 1;
  const bool copy = p.src_cols == p.cols;
  const int sx0 = copy ? x : p.xfirst[x], nx = copy ? 1 : p.xcount[x];
  const int16_t* q = copy ? nullptr : p.xweight + p.xwofs[x];
  const int b0 = (wx + sx0) * CH, half = copy ? 0 : (1 << p.xprec) >> 1;
  for (int r = s.row_lo + wave; r < s.row_hi; r += kAaWaves) {
    RowWindow rw(reinterpret_cast<const uint32_t*>(src_frame + (size_t)r * p.src_step), b0, last_dw);
    uint8_t* out = lds + (size_t)(r - s.row_lo) * CH * kAaTileCols + lane;
    if (copy) {
      const uint32_t v = rw.at(b0);
#pragma unroll
      for (int c = 0; c < CH; c++) out[c * kAaTileCols] = (uint8_t)((v >> (8 * c)) & 255u);
      continue;
    }
    int acc[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) acc[c] = half;
    int b = b0;
    for (int k = 0; k < nx; k++) {
      const uint32_t v = rw.at(b);
      const int a = q[k];
#pragma unroll
      for (int c = 0; c < CH; c++) acc[c] += (int)((v >> (8 * c)) & 255u) * a;
      b += CH;
      rw.advance(b);
    }
#pragma unroll
    for (int c = 0; c < CH; c++) out[c * kAaTileCols] = aa_byte(acc[c], p.xprec);
  }
}

template <int CH, bool WIN>
__device__ __forceinline__ void aa_phase2(const AaParams& p, const FitWindow&, const uint8_t* lds) {
  const int lane = (int)threadIdx.x % kAaTileCols, wave = (int)threadIdx.x / kAaTileCols;
  const int x = (int)blockIdx.x * kAaTileCols + lane;
  if (x >= p.cols) return;
  const AaSpan s = aa_span(p);
  uint8_t* dst_frame = p.dst + (size_t)blockIdx.z * p.dst_frame_stride;
  const bool copy = p.src_rows == p.rows;
  const int half = copy ? 0 : (1 << p.yprec) >> 1;
  for (int y = s.y0 + wave; y <= s.y1; y += kAaWaves) {
    uint8_t* out = dst_frame + (size_t)y * p.dst_step + (size_t)x * CH;
    if (copy) {
      const uint8_t* in = lds + (size_t)(y - s.row_lo) * CH * kAaTileCols + lane;
#pragma unroll
      for (int c = 0; c < CH; c++) out[c] = in[c * kAaTileCols];
      continue;
    }
    const int ny = p.ycount[y];
    const int16_t* q = p.yweight + p.ywofs[y];
    const uint8_t* in = lds + (size_t)(p.yfirst[y] - s.row_lo) * CH * kAaTileCols + lane;
    int acc[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) acc[c] = half;
    for (int j = 0; j < ny; j++) {
      const int a = q[j];
#pragma unroll
      for (int c = 0; c < CH; c++) acc[c] += (int)in[c * kAaTileCols] * a;
      in += CH * kAaTileCols;
    }
#pragma unroll
    for (int c = 0; c < CH; c++) out[c] = aa_byte(acc[c], p.yprec);
  }
}

// ---- the host side: what launch_aa checks beyond the layout (rip_resize_dev.hpp layout_ok) ----

static_assert(kAaMaxSide == kRszMaxSide, "layout_ok's side limit is the resize stage's");

inline bool aa_ok(const AaParams& p) {
  if (p.rows == p.src_rows && p.cols == p.src_cols) return false;  // the identity: nothing, or the linear tables' copy
  if (p.src_rows > kAaMaxFactor * p.rows || p.src_cols > kAaMaxFactor * p.cols) return false;
  if (p.tile_rows != 1 && p.tile_rows != 2 && p.tile_rows != 4 && p.tile_rows != 8) return false;
  if (p.lds_rows < 1 || (size_t)p.lds_rows * kAaTileCols * p.channels > kAaMaxLdsBytes) return false;
  if (p.cols != p.src_cols) {
    if (p.xprec < 1 || p.xprec > kAaMaxPrec) return false;
    for (const void* t : {(const void*)p.xfirst, (const void*)p.xcount, (const void*)p.xwofs})
      if (!t || (reinterpret_cast<uintptr_t>(t) & 3)) return false;
    if (!p.xweight || (reinterpret_cast<uintptr_t>(p.xweight) & 1)) return false;
  }
  if (p.rows != p.src_rows) {
    if (p.yprec < 1 || p.yprec > kAaMaxPrec) return false;
    for (const void* t : {(const void*)p.yfirst, (const void*)p.ycount, (const void*)p.ywofs})
      if (!t || (reinterpret_cast<uintptr_t>(t) & 3)) return false;
    if (!p.yweight || (reinterpret_cast<uintptr_t>(p.yweight) & 1)) return false;
  } else if (p.lds_rows < std::min(p.tile_rows, p.rows)) {
    return false;  // the skipped vertical pass copies the rectangle's own rows
  }
  return true;
}

inline dim3 aa_grid(const AaParams& p) {
  return dim3((unsigned)((p.cols + kAaTileCols - 1) / kAaTileCols), (unsigned)((p.rows + p.tile_rows - 1) / p.tile_rows), (unsigned)p.n_frames);
}

}  // namespace rip
