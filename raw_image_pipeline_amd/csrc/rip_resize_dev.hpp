// rip_resize_dev.hpp -- what the three libraries of the resize stage share: the arithmetic of rip_resize.hip, rip_area.hip and
// rip_fit.hip, once, and the checks their launch functions make.  Included by those three files alone; it adds no symbol to any
// library (device code is inlined into the kernels that name it, host code is inline and hidden).
//
// Each body is the work of one lane of its kernel, with a compile-time switch WIN: false reads all of F, and the origin is the
// constant 0 and the row of F is p.src_cols pixels long, so that the whole-frame kernels are what they were without the switch; true
// reads the window `w` of F (rip_resize.hpp FitWindow).  Pixel (u, v) of the window is pixel (w.x + u, w.y + v) of F: the byte offset
// of a lane's first tap is (w.x + u) * CH from a row start that is 4-byte aligned, at any phase inside its dword.  Rows are read as
// aligned dwords, none beyond the dword that holds the last byte of the row of F (not of the window: the pixels right of the window
// are there to be read, and never used -- the tables clamp at the window's edges, and a clamped second tap has the weight 0 or is
// replaced by the first).  The window itself is never copied.
//   linear_rows<CH, WIN>        the two-tap tables (PARITY.md "Resize"): integer work only
//   mean2_rows<CH, WIN>         the mean (a + b + c + d + 2) >> 2 of every 2 x 2 block; its loads differ with WIN
//   area_rows<CH, WHOLE, WIN>   PARITY.md "Resize: area interpolation": float32, product then sum, in tap order
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rip_area.hpp"
#include "rip_resize.hpp"

namespace rip {
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// n pixels of CH bytes at q: dword stores when `wide` (q is then 4-byte aligned) and all 4 pixels are wanted, else single bytes
template <int CH>
__device__ __forceinline__ void store_pixels(uint8_t* q, const uint8_t v[4 * CH], int n, bool wide) {
  if (wide && n == kRszPxPerLane) {
    uint32_t* q4 = reinterpret_cast<uint32_t*>(q);
#pragma unroll
    for (int k = 0; k < CH; k++)
      q4[k] = (uint32_t)v[4 * k] | ((uint32_t)v[4 * k + 1] << 8) | ((uint32_t)v[4 * k + 2] << 16) | ((uint32_t)v[4 * k + 3] << 24);
  } else {
#pragma unroll
    for (int i = 0; i < kRszPxPerLane * CH; i++)  // constant indices: v[] stays in registers
      if (i < n * CH) q[i] = v[i];
  }
}

// the 2 * CH bytes from byte `b` of a row on, in the low bits of the result: the row as aligned dwords, none read beyond `last_dw`
template <int CH>
__device__ __forceinline__ uint64_t load_taps(const uint32_t* row, int b, int last_dw) {
  const int dw = b >> 2, sh = (b & 3) * 8;
  const uint32_t d0 = row[dw], d1 = row[min(dw + 1, last_dw)];
  uint64_t v = ((uint64_t)d0 | ((uint64_t)d1 << 32)) >> sh;
  if constexpr (CH == 3) {
    if (sh == 24) v |= (uint64_t)row[min(dw + 2, last_dw)] << 40;  // 6 bytes from byte 3 on end in a third dword
  }
  return v;
}

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

// A lane owns 4 consecutive output pixels of one row, a workgroup of 256 lanes covers 1024 of them; the grid's y walks the output
// rows.  Everything that depends on the column alone -- byte offset of the first tap, whether a second tap exists, the two
// weights -- is read from the per-column tables once, in front of the row loop; the per-row tables give the two source rows and
// their weights:
//   h_k = S_k[sx] * a0 + S_k[sx'] * a1 for the rows k = 0, 1;  value = (((b0 * (h_0 >> 4)) >> 16) + ((b1 * (h_1 >> 4)) >> 16) + 2) >> 2
// The two taps of a pixel are 2 or 6 adjacent bytes, read as the two or three aligned dwords that hold them (a dword index beyond
// the row's last dword is clamped to it: it can only hold a second tap that does not exist).
template <int CH, bool WIN>
__device__ __forceinline__ void linear_rows(const ResizeParams& p, const FitWindow& w) {
  const int x0 = ((int)blockIdx.x * kRszBlock + (int)threadIdx.x) * kRszPxPerLane;
  if (x0 >= p.cols) return;
  const int n = min(kRszPxPerLane, p.cols - x0);  // pixels of this lane: 4, or 1 - 3 at the end of a row
  const int wx = WIN ? w.x : 0, wy = WIN ? w.y : 0, frame_cols = WIN ? w.frame_cols : p.src_cols;
  const uint8_t* src_frame = p.src + (size_t)blockIdx.z * p.src_frame_stride;
  uint8_t* dst_frame = p.dst + (size_t)blockIdx.z * p.dst_frame_stride;
  uint8_t v[4 * CH];
#pragma unroll
  for (int i = 0; i < 4 * CH; i++) v[i] = 0;
  // per column, once: the tables are padded to whole lanes and 16-byte aligned (rip_resize.hpp)
  const i32x4 xo = *reinterpret_cast<const i32x4*>(p.xofs + x0);
  const u32x4 al = *reinterpret_cast<const u32x4*>(p.alpha + 2 * x0);  // (a0, a1) of a pixel in one dword
  int off[4], a0[4], a1[4];
  bool two[4];  // a second tap exists: sx + 1 <= C - 1 (else it is the first tap again)
#pragma unroll
  for (int j = 0; j < 4; j++) {
    int sx = xo[j];
    if constexpr (WIN) sx = j < n ? sx : 0;  // the tables' padding is loaded, never used as an offset: it would be one into F
    off[j] = (wx + sx) * CH;
    two[j] = sx + 1 < p.src_cols;
    a0[j] = (int)(int16_t)(al[j] & 0xFFFFu);
    a1[j] = (int)(int16_t)(al[j] >> 16);
  }
  const int last_dw = ((frame_cols * CH + 3) >> 2) - 1;
  for (int y = blockIdx.y; y < p.rows; y += gridDim.y) {
    const int sy0 = wy + p.yofs[2 * y], sy1 = wy + p.yofs[2 * y + 1];
    const int b0 = p.beta[2 * y], b1 = p.beta[2 * y + 1];
    const uint32_t* r0 = reinterpret_cast<const uint32_t*>(src_frame + (size_t)sy0 * p.src_step);
    const uint32_t* r1 = reinterpret_cast<const uint32_t*>(src_frame + (size_t)sy1 * p.src_step);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (j < n) {
        const uint64_t t0 = load_taps<CH>(r0, off[j], last_dw), t1 = load_taps<CH>(r1, off[j], last_dw);
#pragma unroll
        for (int c = 0; c < CH; c++) {
          const int s = two[j] ? 8 * (CH + c) : 8 * c;
          const int h0 = (int)((t0 >> (8 * c)) & 255u) * a0[j] + (int)((t0 >> s) & 255u) * a1[j];
          const int h1 = (int)((t1 >> (8 * c)) & 255u) * a0[j] + (int)((t1 >> s) & 255u) * a1[j];
          v[j * CH + c] = (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
        }
      }
    }
    uint8_t* row = dst_frame + (size_t)y * p.dst_step;
    store_pixels<CH>(row + (size_t)x0 * CH, v, n, (reinterpret_cast<uintptr_t>(row) & 3) == 0);
  }
}

// The geometry of linear_rows; no table is read.  The lane's 4 pixels are the means of 8 consecutive source pixels of two rows.
// All of F: 8 * CH bytes from an 8-byte aligned offset, 2 * CH dwords per row.  A window: 8 * CH bytes from byte (w.x + 2 x0) * CH
// on, at any phase -- 2 * CH + 1 aligned dwords per row, shifted down by the phase of that byte.
template <int CH, bool WIN>
__device__ __forceinline__ void mean2_rows(const ResizeParams& p, const FitWindow& w) {
  const int x0 = ((int)blockIdx.x * kRszBlock + (int)threadIdx.x) * kRszPxPerLane;
  if (x0 >= p.cols) return;
  const int n = min(kRszPxPerLane, p.cols - x0);
  const uint8_t* src_frame = p.src + (size_t)blockIdx.z * p.src_frame_stride;
  uint8_t* dst_frame = p.dst + (size_t)blockIdx.z * p.dst_frame_stride;
  constexpr int kDw = 2 * CH;
  const int b = WIN ? (w.x + 2 * x0) * CH : 0, sh = (b & 3) * 8;
  const int need = ((b & 3) + 2 * n * CH + 3) >> 2;  // dwords that hold a byte of the lane's source pixels: all inside the row of F
  uint8_t v[4 * CH];
#pragma unroll
  for (int i = 0; i < 4 * CH; i++) v[i] = 0;
  for (int y = blockIdx.y; y < p.rows; y += gridDim.y) {
    uint32_t w0[kDw], w1[kDw];
    if constexpr (WIN) {
      const uint8_t* s = src_frame + (size_t)(w.y + 2 * y) * p.src_step;
      const uint32_t* r0 = reinterpret_cast<const uint32_t*>(s) + (b >> 2);
      const uint32_t* r1 = reinterpret_cast<const uint32_t*>(s + p.src_step) + (b >> 2);
      uint32_t l0[kDw + 1], l1[kDw + 1];
#pragma unroll
      for (int k = 0; k <= kDw; k++) {
        l0[k] = k < need ? r0[k] : 0u;
        l1[k] = k < need ? r1[k] : 0u;
      }
#pragma unroll
      for (int k = 0; k < kDw; k++) {
        w0[k] = (uint32_t)((((uint64_t)l0[k + 1] << 32) | l0[k]) >> sh);
        w1[k] = (uint32_t)((((uint64_t)l1[k + 1] << 32) | l1[k]) >> sh);
      }
    } else {
      const uint8_t* s = src_frame + (size_t)(2 * y) * p.src_step + (size_t)x0 * 2 * CH;
      const uint32_t* r0 = reinterpret_cast<const uint32_t*>(s);
      const uint32_t* r1 = reinterpret_cast<const uint32_t*>(s + p.src_step);
#pragma unroll
      for (int k = 0; k < kDw; k++) {
        w0[k] = k < need ? r0[k] : 0u;
        w1[k] = k < need ? r1[k] : 0u;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int c = 0; c < CH; c++) {
        const int i0 = 2 * j * CH + c, i1 = i0 + CH;  // the block's left and right column
        const uint32_t sum = ((w0[i0 >> 2] >> (8 * (i0 & 3))) & 255u) + ((w0[i1 >> 2] >> (8 * (i1 & 3))) & 255u) +
                             ((w1[i0 >> 2] >> (8 * (i0 & 3))) & 255u) + ((w1[i1 >> 2] >> (8 * (i1 & 3))) & 255u);
        v[j * CH + c] = (uint8_t)((sum + 2u) >> 2);
      }
    uint8_t* row = dst_frame + (size_t)y * p.dst_step;
    store_pixels<CH>(row + (size_t)x0 * CH, v, n, (reinterpret_cast<uintptr_t>(row) & 3) == 0);
  }
}

// A workgroup owns a rectangle of 64 x 8 output pixels of one frame.  A lane owns one output column of it: the consecutive source
// columns [sx0, sx0 + nx) and their weights are read from the per-column tables once, in front of the row loop.  A wave takes the
// output rows w, w + 4 of the rectangle and walks the source rows [sy0, sy0 + ny) of each:
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
// read a second time by the next wave, from the caches.  A lane stores the CH bytes of its one pixel as single bytes (a wave's
// stores of a row are 64 * CH consecutive bytes).
template <int CH, bool WHOLE, bool WIN>
__device__ __forceinline__ void area_rows(const AreaParams& p, const FitWindow& w) {
  const int lane = (int)threadIdx.x % kAreaTileCols, wave = (int)threadIdx.x / kAreaTileCols;
  const int x = (int)blockIdx.x * kAreaTileCols + lane;
  if (x >= p.cols) return;
  const int wx = WIN ? w.x : 0, frame_cols = WIN ? w.frame_cols : p.src_cols;
  const uint8_t* src_frame = p.src + (size_t)blockIdx.z * p.src_frame_stride;
  if constexpr (WIN) src_frame += (size_t)w.y * p.src_step;
  uint8_t* dst_frame = p.dst + (size_t)blockIdx.z * p.dst_frame_stride;
  const int last_dw = ((frame_cols * CH + 3) >> 2) - 1;
  const int y_end = min(p.rows, ((int)blockIdx.y + 1) * kAreaTileRows);
  if constexpr (WHOLE) {
    const int kx = p.src_cols / p.cols, ky = p.src_rows / p.rows;
    const int b0 = (wx + x * kx) * CH;
    for (int y = (int)blockIdx.y * kAreaTileRows + wave; y < y_end; y += kAreaWaves) {
      uint32_t sum[CH];
#pragma unroll
      for (int c = 0; c < CH; c++) sum[c] = 0u;
      for (int j = 0; j < ky; j++) {
        RowWindow rw(reinterpret_cast<const uint32_t*>(src_frame + (size_t)(y * ky + j) * p.src_step), b0, last_dw);
        int b = b0;
        for (int k = 0; k < kx; k++) {
          const uint32_t v = rw.at(b);
#pragma unroll
          for (int c = 0; c < CH; c++) sum[c] += (v >> (8 * c)) & 255u;
          b += CH;
          rw.advance(b);
        }
      }
      uint8_t* q = dst_frame + (size_t)y * p.dst_step + (size_t)x * CH;
#pragma unroll
      for (int c = 0; c < CH; c++) q[c] = to_byte((float)sum[c] * p.scale);
    }
  } else {
    const int sx0 = p.xfirst[x], nx = p.xcount[x];
    const float* wxs = p.xweight + p.xwofs[x];
    const int b0 = (wx + sx0) * CH;
    for (int y = (int)blockIdx.y * kAreaTileRows + wave; y < y_end; y += kAreaWaves) {
      const int sy0 = p.yfirst[y], ny = p.ycount[y];
      const float* wys = p.yweight + p.ywofs[y];
      float acc[CH];
#pragma unroll
      for (int c = 0; c < CH; c++) acc[c] = 0.f;
      for (int j = 0; j < ny; j++) {
        RowWindow rw(reinterpret_cast<const uint32_t*>(src_frame + (size_t)(sy0 + j) * p.src_step), b0, last_dw);
        float buf[CH];
#pragma unroll
        for (int c = 0; c < CH; c++) buf[c] = 0.f;
        int b = b0;
        for (int k = 0; k < nx; k++) {
          const uint32_t v = rw.at(b);
          const float a = wxs[k];
#pragma unroll
          for (int c = 0; c < CH; c++) {
            const float prod = (float)((v >> (8 * c)) & 255u) * a;
            buf[c] = buf[c] + prod;
          }
          b += CH;
          rw.advance(b);
        }
        const float bj = wys[j];
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

// ---- the host side: what a launch function checks before it launches, and the launch with its record ----

static_assert(kAreaMaxSide == kRszMaxSide, "one layout check serves both parameter structs");

inline FitWindow whole_frame(int src_rows, int src_cols) { return FitWindow{0, 0, src_cols, src_rows}; }

// The layout rules of rip_resize.hpp / rip_area.hpp for a window `w` of F (P: ResizeParams or AreaParams): source alignment, pitch
// against the row of F, frame stride, frame and channel counts, destination pitch, every side within 1 .. kRszMaxSide, the window
// inside F.
template <typename P>
inline bool layout_ok(const P& p, const FitWindow& w) {
  if (!p.src || !p.dst || p.n_frames < 1 || p.n_frames > 65535 || (p.channels != 1 && p.channels != 3)) return false;
  for (int side : {p.src_rows, p.src_cols, p.rows, p.cols, w.frame_rows, w.frame_cols})
    if (side < 1 || side > kRszMaxSide) return false;
  if (w.x < 0 || w.y < 0 || w.x > w.frame_cols - p.src_cols || w.y > w.frame_rows - p.src_rows) return false;  // the window lies inside F
  if ((reinterpret_cast<uintptr_t>(p.src) | p.src_step | p.src_frame_stride) & 3) return false;
  if (p.src_step < (((size_t)w.frame_cols * p.channels + 3) & ~(size_t)3) || p.src_frame_stride < p.src_step * (size_t)w.frame_rows) return false;
  return p.dst_step >= (size_t)p.cols * p.channels;
}

// what launch_resize and launch_fit_resize ask beyond the layout: an area2 flag that matches the sizes and, unless it is set, the
// four tables at their alignments.  *mean2: the 2 x 2 mean is the kernel.
inline bool linear_ok(const ResizeParams& p, bool* mean2) {
  *mean2 = p.src_rows == 2 * p.rows && p.src_cols == 2 * p.cols;
  if (*mean2 != (p.area2 != 0)) return false;
  return *mean2 || (p.xofs && p.alpha && p.yofs && p.beta && !((reinterpret_cast<uintptr_t>(p.xofs) | reinterpret_cast<uintptr_t>(p.alpha)) & 15) &&
                    !(reinterpret_cast<uintptr_t>(p.yofs) & 3) && !(reinterpret_cast<uintptr_t>(p.beta) & 1));
}

// what launch_area_reduce and launch_fit_area ask beyond the layout.  *whole: the block-sum kernel is the one.
inline bool area_ok(const AreaParams& p, bool* whole) {
  *whole = false;
  if (p.rows > p.src_rows || p.cols > p.src_cols) return false;                                             // an upscale
  if (p.src_rows > kAreaMaxFactor * p.rows || p.src_cols > kAreaMaxFactor * p.cols) return false;
  if (p.rows == p.src_rows && p.cols == p.src_cols) return false;                                           // the identity: nothing, or the linear tables'
  if (p.src_rows == 2 * p.rows && p.src_cols == 2 * p.cols) return false;                                   // the 2 x 2 mean of the linear launches
  *whole = p.src_rows % p.rows == 0 && p.src_cols % p.cols == 0;
  if (*whole != (p.whole != 0)) return false;
  if (*whole) return p.scale > 0.f;
  for (const void* t : {(const void*)p.xfirst, (const void*)p.xcount, (const void*)p.xwofs, (const void*)p.xweight, (const void*)p.yfirst,
                        (const void*)p.ycount, (const void*)p.ywofs, (const void*)p.yweight})
    if (!t || (reinterpret_cast<uintptr_t>(t) & 3)) return false;
  return true;
}

// grid of the kernels with linear_rows' geometry, and of those with area_rows'
inline dim3 rsz_grid(int rows, int cols, int n_frames) {
  return dim3((unsigned)((cols + kRszPxPerBlock - 1) / kRszPxPerBlock), (unsigned)(rows < 65535 ? rows : 65535), (unsigned)n_frames);
}
inline dim3 area_grid(int rows, int cols, int n_frames) {
  return dim3((unsigned)((cols + kAreaTileCols - 1) / kAreaTileCols), (unsigned)((rows + kAreaTileRows - 1) / kAreaTileRows), (unsigned)n_frames);
}

// A kernel instantiation with its name as the demangler prints it, without namespaces: RIP_NAMED_KERNEL(resize_kernel<3, false>)
template <typename... A>
struct NamedKernel {
  void (*fn)(A...);
  const char* name;
};
#define RIP_NAMED_KERNEL(...) {(__VA_ARGS__), #__VA_ARGS__}

// launches variants[channels == 3][flag] and writes the launch record
template <typename... A>
inline void launch_variant(const NamedKernel<A...> (&variants)[2][2], int channels, bool flag, dim3 grid, int block, hipStream_t stream,
                           LaunchInfo* info, const A&... args) {
  const NamedKernel<A...>& k = variants[channels == 3][flag];
  hipLaunchKernelGGL(k.fn, grid, dim3(block), 0, stream, args...);
  if (info) *info = LaunchInfo{k.name, grid.x, grid.y, (unsigned)block};
}

}  // namespace rip
