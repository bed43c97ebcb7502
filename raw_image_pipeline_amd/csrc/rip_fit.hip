// rip_fit.hip -- the resize stage on a window of F, and the letterbox bands (rip_set_output_roi / rip_set_output_fit, rip_fit.hpp;
// PARITY.md "Resize: window and fit").  Built into librip_fit_hip.so.
//
// The three window kernels do the arithmetic of rip_resize.hip and rip_area.hip -- same tables, built for the window's size, same
// integer and float32 statements in the same order, same lane and workgroup geometry -- and differ in where they read: pixel
// (u, v) of the window is pixel (x + u, y + v) of F, so the byte offset of a lane's first tap is (x + u) * CH from a row start that
// is 4-byte aligned, at any phase inside its dword.  Rows are read as aligned dwords, none beyond the dword that holds the last
// byte of the row of F (not of the window: the pixels right of the window are there to be read, and never used -- the tables
// clamp at the window's edges, and a clamped second tap has the weight 0 or is replaced by the first).  The window itself is never
// copied.  The 2 x 2 mean shifts the dwords it has loaded by the phase; rip_resize.hip's aligned kernel is not involved.
//
// fit_pad_kernel writes the pad colour to every pixel of F' outside the picture: a lane owns 4 consecutive pixels of a row, whole
// dwords where the row start is 4-byte aligned and all 4 are pad, single bytes otherwise.  Lanes inside the picture leave at once.
// Nothing is written at or beyond column `cols` of any row by any kernel here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rip_fit.hpp"

namespace rip {
namespace {
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

// the two-tap tables on a window (rip_resize.hip resize_kernel<CH, false>)
template <int CH>
__global__ __launch_bounds__(kRszBlock) void fit_linear_kernel(ResizeParams p, FitWindow w) {
  const int x0 = ((int)blockIdx.x * kRszBlock + (int)threadIdx.x) * kRszPxPerLane;
  if (x0 >= p.cols) return;
  const int n = min(kRszPxPerLane, p.cols - x0);
  const uint8_t* src_frame = p.src + (size_t)blockIdx.z * p.src_frame_stride;
  uint8_t* dst_frame = p.dst + (size_t)blockIdx.z * p.dst_frame_stride;
  uint8_t v[4 * CH];
#pragma unroll
  for (int i = 0; i < 4 * CH; i++) v[i] = 0;
  const i32x4 xo = *reinterpret_cast<const i32x4*>(p.xofs + x0);
  const u32x4 al = *reinterpret_cast<const u32x4*>(p.alpha + 2 * x0);
  int off[4], a0[4], a1[4];
  bool two[4];  // a second tap exists inside the window
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int sx = j < n ? xo[j] : 0;  // the tables' padding is loaded, never used as an offset
    off[j] = (w.x + sx) * CH;
    two[j] = sx + 1 < p.src_cols;
    a0[j] = (int)(int16_t)(al[j] & 0xFFFFu);
    a1[j] = (int)(int16_t)(al[j] >> 16);
  }
  const int last_dw = ((w.frame_cols * CH + 3) >> 2) - 1;
  for (int y = blockIdx.y; y < p.rows; y += gridDim.y) {
    const int sy0 = w.y + p.yofs[2 * y], sy1 = w.y + p.yofs[2 * y + 1];
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

// the 2 x 2 mean on a window: the lane's 4 pixels are the means of 8 consecutive source pixels of two rows, 8 * CH bytes from byte
// (x + 2 x0) * CH on -- 2 * CH + 1 aligned dwords shifted down by the phase of that byte
template <int CH>
__global__ __launch_bounds__(kRszBlock) void fit_mean2_kernel(ResizeParams p, FitWindow w) {
  const int x0 = ((int)blockIdx.x * kRszBlock + (int)threadIdx.x) * kRszPxPerLane;
  if (x0 >= p.cols) return;
  const int n = min(kRszPxPerLane, p.cols - x0);
  const uint8_t* src_frame = p.src + (size_t)blockIdx.z * p.src_frame_stride;
  uint8_t* dst_frame = p.dst + (size_t)blockIdx.z * p.dst_frame_stride;
  constexpr int kDw = 2 * CH;
  const int b = (w.x + 2 * x0) * CH, sh = (b & 3) * 8;
  const int need = ((b & 3) + 2 * n * CH + 3) >> 2;  // dwords that hold a byte of the lane's source pixels: all inside the row of F
  uint8_t v[4 * CH];
#pragma unroll
  for (int i = 0; i < 4 * CH; i++) v[i] = 0;
  for (int y = blockIdx.y; y < p.rows; y += gridDim.y) {
    const uint8_t* s = src_frame + (size_t)(w.y + 2 * y) * p.src_step;
    const uint32_t* r0 = reinterpret_cast<const uint32_t*>(s) + (b >> 2);
    const uint32_t* r1 = reinterpret_cast<const uint32_t*>(s + p.src_step) + (b >> 2);
    uint32_t l0[kDw + 1], l1[kDw + 1], w0[kDw], w1[kDw];
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

// The bytes of a row from byte `b` on, read as aligned dwords in ascending order, none beyond `last_dw` (rip_area.hip)
struct RowWindow {
  const uint32_t* row;
  int dw, last_dw;
  uint32_t lo, hi;
  __device__ __forceinline__ RowWindow(const uint32_t* r, int b, int last) : row(r), dw(b >> 2), last_dw(last) {
    lo = row[dw];
    hi = row[min(dw + 1, last_dw)];
  }
  __device__ __forceinline__ uint32_t at(int b) const { return (uint32_t)((((uint64_t)hi << 32) | lo) >> ((b & 3) * 8)); }
  __device__ __forceinline__ void advance(int b) {
    if ((b >> 2) != dw) {
      dw++;
      lo = hi;
      hi = row[min(dw + 1, last_dw)];
    }
  }
};

__device__ __forceinline__ uint8_t to_byte(float acc) { return (uint8_t)(int)fminf(fmaxf(rintf(acc), 0.f), 255.f); }

// the area interpolation on a window (rip_area.hip area_reduce_kernel<CH, WHOLE>)
template <int CH, bool WHOLE>
__global__ __launch_bounds__(kAreaBlock) void fit_area_kernel(AreaParams p, FitWindow w) {
  const int lane = (int)threadIdx.x % kAreaTileCols, wave = (int)threadIdx.x / kAreaTileCols;
  const int x = (int)blockIdx.x * kAreaTileCols + lane;
  if (x >= p.cols) return;
  const uint8_t* src_frame = p.src + (size_t)blockIdx.z * p.src_frame_stride + (size_t)w.y * p.src_step;
  uint8_t* dst_frame = p.dst + (size_t)blockIdx.z * p.dst_frame_stride;
  const int last_dw = ((w.frame_cols * CH + 3) >> 2) - 1;
  const int y_end = min(p.rows, ((int)blockIdx.y + 1) * kAreaTileRows);
  if constexpr (WHOLE) {
    const int kx = p.src_cols / p.cols, ky = p.src_rows / p.rows;
    const int b0 = (w.x + x * kx) * CH;
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
    const float* wx = p.xweight + p.xwofs[x];
    const int b0 = (w.x + sx0) * CH;
    for (int y = (int)blockIdx.y * kAreaTileRows + wave; y < y_end; y += kAreaWaves) {
      const int sy0 = p.yfirst[y], ny = p.ycount[y];
      const float* wy = p.yweight + p.ywofs[y];
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
          const float a = wx[k];
#pragma unroll
          for (int c = 0; c < CH; c++) {
            const float prod = (float)((v >> (8 * c)) & 255u) * a;
            buf[c] = buf[c] + prod;
          }
          b += CH;
          rw.advance(b);
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

template <int CH>
__global__ __launch_bounds__(kRszBlock) void fit_pad_kernel(FitPadParams p) {
  const int x0 = ((int)blockIdx.x * kRszBlock + (int)threadIdx.x) * kRszPxPerLane;
  if (x0 >= p.cols) return;
  const int n = min(kRszPxPerLane, p.cols - x0);
  const int px1 = p.pic_x + p.pic_w, py1 = p.pic_y + p.pic_h;
  const bool in_cols = x0 >= p.pic_x && x0 + n <= px1;     // every pixel of the lane lies in the picture's columns
  const bool out_cols = x0 + n <= p.pic_x || x0 >= px1;    // none does
  uint8_t* dst_frame = p.dst + (size_t)blockIdx.z * p.dst_frame_stride;
  uint8_t v[4 * CH];
#pragma unroll
  for (int i = 0; i < 4 * CH; i++) v[i] = p.color[i % CH];
  for (int y = blockIdx.y; y < p.rows; y += gridDim.y) {
    const bool in_rows = y >= p.pic_y && y < py1;
    if (in_rows && in_cols) continue;
    uint8_t* row = dst_frame + (size_t)y * p.dst_step;
    uint8_t* q = row + (size_t)x0 * CH;
    if (!in_rows || out_cols) {
      store_pixels<CH>(q, v, n, (reinterpret_cast<uintptr_t>(row) & 3) == 0);
    } else {  // the lane straddles an edge of the picture: the pixels outside it, byte by byte
#pragma unroll
      for (int j = 0; j < kRszPxPerLane; j++)
        if (j < n && (x0 + j < p.pic_x || x0 + j >= px1)) {
#pragma unroll
          for (int c = 0; c < CH; c++) q[j * CH + c] = v[c];
        }
    }
  }
}

bool layout_ok(const uint8_t* src, size_t src_step, size_t src_frame_stride, const uint8_t* dst, size_t dst_step, int src_rows, int src_cols, int cols,
               int channels, int n_frames, const FitWindow& w) {
  if (!src || !dst || n_frames < 1 || n_frames > 65535 || (channels != 1 && channels != 3)) return false;
  if (w.x < 0 || w.y < 0 || w.frame_cols < 1 || w.frame_rows < 1 || w.frame_cols > kRszMaxSide || w.frame_rows > kRszMaxSide) return false;
  if (src_cols < 1 || src_rows < 1 || w.x > w.frame_cols - src_cols || w.y > w.frame_rows - src_rows) return false;  // the window lies inside F
  if ((reinterpret_cast<uintptr_t>(src) | src_step | src_frame_stride) & 3) return false;
  if (src_step < (((size_t)w.frame_cols * channels + 3) & ~(size_t)3) || src_frame_stride < src_step * (size_t)w.frame_rows) return false;
  return dst_step >= (size_t)cols * channels;
}
}  // namespace

bool launch_fit_resize(const ResizeParams& p, const FitWindow& w, hipStream_t stream, FitLaunchInfo* info) {
  for (int side : {p.src_rows, p.src_cols, p.rows, p.cols})
    if (side < 1 || side > kRszMaxSide) return false;
  if (!layout_ok(p.src, p.src_step, p.src_frame_stride, p.dst, p.dst_step, p.src_rows, p.src_cols, p.cols, p.channels, p.n_frames, w)) return false;
  const bool mean2 = p.src_rows == 2 * p.rows && p.src_cols == 2 * p.cols;
  if (mean2 != (p.area2 != 0)) return false;
  if (!mean2 && (!p.xofs || !p.alpha || !p.yofs || !p.beta || ((reinterpret_cast<uintptr_t>(p.xofs) | reinterpret_cast<uintptr_t>(p.alpha)) & 15) ||
                 (reinterpret_cast<uintptr_t>(p.yofs) & 3) || (reinterpret_cast<uintptr_t>(p.beta) & 1)))
    return false;
  const dim3 grid((unsigned)((p.cols + kRszPxPerBlock - 1) / kRszPxPerBlock), (unsigned)(p.rows < 65535 ? p.rows : 65535), (unsigned)p.n_frames);
  const char* name;
  if (p.channels == 1) {
    if (mean2) {
      hipLaunchKernelGGL((fit_mean2_kernel<1>), grid, dim3(kRszBlock), 0, stream, p, w);
      name = "fit_mean2_kernel<1>";
    }
    else {
      hipLaunchKernelGGL((fit_linear_kernel<1>), grid, dim3(kRszBlock), 0, stream, p, w);
      name = "fit_linear_kernel<1>";
    }
  } else {
    if (mean2) {
      hipLaunchKernelGGL((fit_mean2_kernel<3>), grid, dim3(kRszBlock), 0, stream, p, w);
      name = "fit_mean2_kernel<3>";
    }
    else {
      hipLaunchKernelGGL((fit_linear_kernel<3>), grid, dim3(kRszBlock), 0, stream, p, w);
      name = "fit_linear_kernel<3>";
    }
  }
  if (info) *info = FitLaunchInfo{name, grid.x, grid.y, (unsigned)kRszBlock};
  return true;
}

bool launch_fit_area(const AreaParams& p, const FitWindow& w, hipStream_t stream, FitLaunchInfo* info) {
  for (int side : {p.src_rows, p.src_cols, p.rows, p.cols})
    if (side < 1 || side > kAreaMaxSide) return false;
  if (!layout_ok(p.src, p.src_step, p.src_frame_stride, p.dst, p.dst_step, p.src_rows, p.src_cols, p.cols, p.channels, p.n_frames, w)) return false;
  if (p.rows > p.src_rows || p.cols > p.src_cols) return false;                                             // an upscale
  if (p.src_rows > kAreaMaxFactor * p.rows || p.src_cols > kAreaMaxFactor * p.cols) return false;
  if (p.rows == p.src_rows && p.cols == p.src_cols) return false;                                           // the identity is the linear tables'
  if (p.src_rows == 2 * p.rows && p.src_cols == 2 * p.cols) return false;                                   // the 2 x 2 mean of launch_fit_resize
  const bool whole = p.src_rows % p.rows == 0 && p.src_cols % p.cols == 0;
  if (whole != (p.whole != 0)) return false;
  if (whole) {
    if (!(p.scale > 0.f)) return false;
  } else {
    for (const void* t : {(const void*)p.xfirst, (const void*)p.xcount, (const void*)p.xwofs, (const void*)p.xweight, (const void*)p.yfirst,
                          (const void*)p.ycount, (const void*)p.ywofs, (const void*)p.yweight})
      if (!t || (reinterpret_cast<uintptr_t>(t) & 3)) return false;
  }
  const dim3 grid((unsigned)((p.cols + kAreaTileCols - 1) / kAreaTileCols), (unsigned)((p.rows + kAreaTileRows - 1) / kAreaTileRows), (unsigned)p.n_frames);
  const char* name;
  if (p.channels == 1) {
    if (whole) {
      hipLaunchKernelGGL((fit_area_kernel<1, true>), grid, dim3(kAreaBlock), 0, stream, p, w);
      name = "fit_area_kernel<1, true>";
    }
    else {
      hipLaunchKernelGGL((fit_area_kernel<1, false>), grid, dim3(kAreaBlock), 0, stream, p, w);
      name = "fit_area_kernel<1, false>";
    }
  } else {
    if (whole) {
      hipLaunchKernelGGL((fit_area_kernel<3, true>), grid, dim3(kAreaBlock), 0, stream, p, w);
      name = "fit_area_kernel<3, true>";
    }
    else {
      hipLaunchKernelGGL((fit_area_kernel<3, false>), grid, dim3(kAreaBlock), 0, stream, p, w);
      name = "fit_area_kernel<3, false>";
    }
  }
  if (info) *info = FitLaunchInfo{name, grid.x, grid.y, (unsigned)kAreaBlock};
  return true;
}

bool launch_fit_pad(const FitPadParams& p, hipStream_t stream, FitLaunchInfo* info) {
  if (!p.dst || p.n_frames < 1 || p.n_frames > 65535 || (p.channels != 1 && p.channels != 3)) return false;
  if (p.rows < 1 || p.cols < 1 || p.rows > kRszMaxSide || p.cols > kRszMaxSide) return false;
  if (p.pic_w < 1 || p.pic_h < 1 || p.pic_x < 0 || p.pic_y < 0 || p.pic_x > p.cols - p.pic_w || p.pic_y > p.rows - p.pic_h) return false;
  if (p.pic_w == p.cols && p.pic_h == p.rows) return false;  // no band
  if (p.dst_step < (size_t)p.cols * p.channels) return false;
  const dim3 grid((unsigned)((p.cols + kRszPxPerBlock - 1) / kRszPxPerBlock), (unsigned)(p.rows < 65535 ? p.rows : 65535), (unsigned)p.n_frames);
  if (p.channels == 1) hipLaunchKernelGGL((fit_pad_kernel<1>), grid, dim3(kRszBlock), 0, stream, p);
  else hipLaunchKernelGGL((fit_pad_kernel<3>), grid, dim3(kRszBlock), 0, stream, p);
  if (info) *info = FitLaunchInfo{p.channels == 1 ? "fit_pad_kernel<1>" : "fit_pad_kernel<3>", grid.x, grid.y, (unsigned)kRszBlock};
  return true;
}

}  // namespace rip
