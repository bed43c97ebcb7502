// rip_area.hip -- the resize stage under "area" interpolation (rip_set_output_interpolation, rip_area.hpp): cv::resize(F, size,
// INTER_AREA) for downscales of the pipeline's final 8-bit image of 1 or 3 interleaved channels, one launch per batch slice.  Built
// into librip_area_hip.so.
//
// A workgroup owns a rectangle of 64 x 8 output pixels of one frame.  A lane owns one output column of it: the consecutive source
// columns [sx0, sx0 + nx) and their weights are read from the per-column tables once, in front of the row loop.  A wave takes the
// output rows w, w + 4 of the rectangle and walks the source rows [sy0, sy0 + ny) of each (PARITY.md "Resize: area interpolation"):
//   general:  buf_j = ((0 + S[sy_j][sx_0] a_0) + S[sy_j][sx_1] a_1) + ...;  acc = b_0 buf_0, acc = acc + b_j buf_j;  every product and
//             every sum rounded to float32 (-ffp-contract=off: no fma), in tap order
//   WHOLE:    sum = the integer sum of the ky x kx block;  acc = (float)sum * scale
//   value = clamp(round_half_even(acc), 0, 255).  No division.
// buf_j depends on the source row and the column alone, so the boundary row two output rows share gives both the same buf.
//
// Traffic.  The 64 lanes of a wave own 64 consecutive output columns, and the tap lists of neighbouring columns are adjacent (they
// share at most the boundary pixel): in one source row the wave reads every dword of one contiguous span -- about 64 * C / W * CH
// bytes, 768 at a factor of 4 with 3 channels -- so every cache line inside the span is used whole while it sits in the CU's L1, and
// only the partly covered line at either end is shared with the neighbouring workgroup.  A lane walks its part of the span as
// aligned dwords, each loaded once per source row: the pixel's bytes come out of a 64-bit window of two neighbouring dwords (a dword
// index beyond the row's last dword is clamped to it: it can only hold bytes nobody uses).  A source row two output rows share is
// read a second time by the next wave, from the caches.  Source rows are 4-byte aligned (rip_area.hpp).
//
// The destination is the caller's, at any alignment: a lane stores the CH bytes of its one pixel as single bytes (a wave's stores of
// a row are 64 * CH consecutive bytes).  Nothing is written at or beyond column `cols` of any row.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rip_area.hpp"

namespace rip {
namespace {

// The bytes of a row from byte `b` on, read as aligned dwords in ascending order, none beyond `last_dw`
struct RowWindow {
  const uint32_t* row;
  int dw, last_dw;
  uint32_t lo, hi;
  __device__ __forceinline__ RowWindow(const uint32_t* r, int b, int last) : row(r), dw(b >> 2), last_dw(last) {
    lo = row[dw];
    hi = row[min(dw + 1, last_dw)];
  }
  // the 4 bytes at byte b (b >> 2 == dw), lowest first
  __device__ __forceinline__ uint32_t at(int b) const { return (uint32_t)((((uint64_t)hi << 32) | lo) >> ((b & 3) * 8)); }
  // moves on to byte b: at most one dword further
  __device__ __forceinline__ void advance(int b) {
    if ((b >> 2) != dw) {
      dw++;
      lo = hi;
      hi = row[min(dw + 1, last_dw)];
    }
  }
};

__device__ __forceinline__ uint8_t to_byte(float acc) { return (uint8_t)(int)fminf(fmaxf(rintf(acc), 0.f), 255.f); }

template <int CH, bool WHOLE>
__global__ __launch_bounds__(kAreaBlock) void area_reduce_kernel(AreaParams p) {
  const int lane = (int)threadIdx.x % kAreaTileCols, wave = (int)threadIdx.x / kAreaTileCols;
  const int x = (int)blockIdx.x * kAreaTileCols + lane;
  if (x >= p.cols) return;
  const uint8_t* src_frame = p.src + (size_t)blockIdx.z * p.src_frame_stride;
  uint8_t* dst_frame = p.dst + (size_t)blockIdx.z * p.dst_frame_stride;
  const int last_dw = ((p.src_cols * CH + 3) >> 2) - 1;
  const int y_end = min(p.rows, ((int)blockIdx.y + 1) * kAreaTileRows);
  if constexpr (WHOLE) {
    const int kx = p.src_cols / p.cols, ky = p.src_rows / p.rows;
    const int b0 = x * kx * CH;
    for (int y = (int)blockIdx.y * kAreaTileRows + wave; y < y_end; y += kAreaWaves) {
      uint32_t sum[CH];
#pragma unroll
      for (int c = 0; c < CH; c++) sum[c] = 0u;
      for (int j = 0; j < ky; j++) {
        RowWindow w(reinterpret_cast<const uint32_t*>(src_frame + (size_t)(y * ky + j) * p.src_step), b0, last_dw);
        int b = b0;
        for (int k = 0; k < kx; k++) {
          const uint32_t v = w.at(b);
#pragma unroll
          for (int c = 0; c < CH; c++) sum[c] += (v >> (8 * c)) & 255u;
          b += CH;
          w.advance(b);
        }
      }
      uint8_t* q = dst_frame + (size_t)y * p.dst_step + (size_t)x * CH;
#pragma unroll
      for (int c = 0; c < CH; c++) q[c] = to_byte((float)sum[c] * p.scale);
    }
  } else {
    const int sx0 = p.xfirst[x], nx = p.xcount[x];
    const float* wx = p.xweight + p.xwofs[x];
    const int b0 = sx0 * CH;
    for (int y = (int)blockIdx.y * kAreaTileRows + wave; y < y_end; y += kAreaWaves) {
      const int sy0 = p.yfirst[y], ny = p.ycount[y];
      const float* wy = p.yweight + p.ywofs[y];
      float acc[CH];
#pragma unroll
      for (int c = 0; c < CH; c++) acc[c] = 0.f;
      for (int j = 0; j < ny; j++) {
        RowWindow w(reinterpret_cast<const uint32_t*>(src_frame + (size_t)(sy0 + j) * p.src_step), b0, last_dw);
        float buf[CH];
#pragma unroll
        for (int c = 0; c < CH; c++) buf[c] = 0.f;
        int b = b0;
        for (int k = 0; k < nx; k++) {
          const uint32_t v = w.at(b);
          const float a = wx[k];
#pragma unroll
          for (int c = 0; c < CH; c++) {
            const float prod = (float)((v >> (8 * c)) & 255u) * a;
            buf[c] = buf[c] + prod;
          }
          b += CH;
          w.advance(b);
        }
        const float bj = wy[j];
#pragma unroll
        for (int c = 0; c < CH; c++) {
          const float prod = bj * buf[c];
          acc[c] = j == 0 ? prod : acc[c] + prod;
        }
      }
      uint8_t* q = dst_frame + (size_t)y * p.dst_step + (size_t)x * CH;
#pragma unroll
      for (int c = 0; c < CH; c++) q[c] = to_byte(acc[c]);
    }
  }
}

template <int CH, bool WHOLE>
void launch(const AreaParams& p, hipStream_t stream, const char* name, AreaLaunchInfo* info) {
  const dim3 grid((unsigned)((p.cols + kAreaTileCols - 1) / kAreaTileCols), (unsigned)((p.rows + kAreaTileRows - 1) / kAreaTileRows), (unsigned)p.n_frames);
  hipLaunchKernelGGL((area_reduce_kernel<CH, WHOLE>), grid, dim3(kAreaBlock), 0, stream, p);
  if (info) *info = AreaLaunchInfo{name, grid.x, grid.y, (unsigned)kAreaBlock};
}
}  // namespace

bool launch_area_reduce(const AreaParams& p, hipStream_t stream, AreaLaunchInfo* info) {
  if (!p.src || !p.dst || p.n_frames < 1 || p.n_frames > 65535 || (p.channels != 1 && p.channels != 3)) return false;
  for (int side : {p.src_rows, p.src_cols, p.rows, p.cols})
    if (side < 1 || side > kAreaMaxSide) return false;
  if (p.rows > p.src_rows || p.cols > p.src_cols) return false;                                             // an upscale
  if (p.src_rows > kAreaMaxFactor * p.rows || p.src_cols > kAreaMaxFactor * p.cols) return false;
  if (p.rows == p.src_rows && p.cols == p.src_cols) return false;                                           // the identity launches nothing
  if (p.src_rows == 2 * p.rows && p.src_cols == 2 * p.cols) return false;                                   // the 2 x 2 mean of rip_resize.hpp
  if ((reinterpret_cast<uintptr_t>(p.src) | p.src_step | p.src_frame_stride) & 3) return false;
  if (p.src_step < (((size_t)p.src_cols * p.channels + 3) & ~(size_t)3) || p.src_frame_stride < p.src_step * (size_t)p.src_rows) return false;
  if (p.dst_step < (size_t)p.cols * p.channels) return false;
  const bool whole = p.src_rows % p.rows == 0 && p.src_cols % p.cols == 0;
  if (whole != (p.whole != 0)) return false;
  if (whole) {
    if (!(p.scale > 0.f)) return false;
  } else {
    for (const void* t : {(const void*)p.xfirst, (const void*)p.xcount, (const void*)p.xwofs, (const void*)p.xweight, (const void*)p.yfirst,
                          (const void*)p.ycount, (const void*)p.ywofs, (const void*)p.yweight})
      if (!t || (reinterpret_cast<uintptr_t>(t) & 3)) return false;
  }
  if (p.channels == 1) {
    if (whole) launch<1, true>(p, stream, "area_reduce_kernel<1, true>", info);
    else launch<1, false>(p, stream, "area_reduce_kernel<1, false>", info);
  } else {
    if (whole) launch<3, true>(p, stream, "area_reduce_kernel<3, true>", info);
    else launch<3, false>(p, stream, "area_reduce_kernel<3, false>", info);
  }
  return true;
}

}  // namespace rip
