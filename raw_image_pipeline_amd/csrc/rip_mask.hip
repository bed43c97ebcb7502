// rip_mask.hip -- valid-pixel masks (rip_set_rect_mask, rip_mask.hpp; PARITY.md "Rect mask").  Built into librip_mask_hip.so.
//
// rect_mask_kernel<BINARY>: the coverage mask M = cv::remap(white, map_x, map_y, INTER_LINEAR, BORDER_CONSTANT 0) of an all-255
// image of src_rows x src_cols, from the interleaved float maps alone -- 8 bytes read and 1 written per pixel, no source image.
// A white source turns the four-weight sum of the remap (rip_remap_dev.hpp remap_pixel) into a product: with (sx, fx), (sy, fy) the
// quantised tap position (round_map: the remap kernels' own quantiser) the weight of the taps inside the source is X * Y / 1024,
// X = (32 - fx) [0 <= sx < C] + fx [0 <= sx + 1 < C], Y alike, and M = (255 * 32 * X * Y + 2^14) >> 15: an integer identity, so the
// mask equals the remap byte for byte.  BINARY writes (M == 255) ? 255 : 0.
//
// A lane owns 4 consecutive pixels of one row: it reads their 32 map bytes as two 16-byte loads where the row's first entry is
// 16-byte aligned (a map row starts at y * dcols * 8 bytes: the lanes of a row start 32 bytes apart, so the test is per row and
// wave-uniform) and as four 8-byte loads otherwise, and writes one dword where the mask row is 4-byte aligned; the last lane of a
// row reads and writes the 1 - 3 pixels that are left one by one.  Nothing is read beyond the last map entry of a row and nothing is
// written at or beyond dcols of a row.  Integer work only behind round_map, no LDS.
//
// mask_threshold_kernel: v = (v == 255) ? 255 : 0 in place on a pitched image, one dword per lane -- the `valid` mode's threshold
// behind a head's resize, which filtered the coverage.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rip_mask.hpp"
#include "rip_round_map.hpp"

namespace rip {
namespace {
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// weight, out of 32, of the taps s and s + 1 that lie inside [0, size): q is the tap position in 1/32 pixel
__device__ __forceinline__ int inside_weight(int q, int size) {
  int s = q >> 5;
  s = s < -32768 ? -32768 : (s > 32767 ? 32767 : s);  // cv::remap keeps tap positions as int16, saturated
  const int f = q & 31;
  return ((unsigned)s < (unsigned)size ? 32 - f : 0) + ((unsigned)(s + 1) < (unsigned)size ? f : 0);
}

template <bool BINARY>
__device__ __forceinline__ uint32_t mask_value(float mx, float my, int src_rows, int src_cols) {
  const int X = inside_weight(round_map(mx), src_cols), Y = inside_weight(round_map(my), src_rows);
  const uint32_t m = (uint32_t)(255 * 32 * X * Y + 16384) >> 15;  // X, Y <= 32: at most 255
  return BINARY ? (m == 255u ? 255u : 0u) : m;
}
}  // namespace

template <bool BINARY>
__global__ __launch_bounds__(kMaskBlock) void rect_mask_kernel(RectMaskParams p) {
  const int x0 = ((int)blockIdx.x * kMaskBlock + (int)threadIdx.x) * kMaskPxPerLane;
  if (x0 >= p.dcols) return;
  const int n = min(kMaskPxPerLane, p.dcols - x0);  // pixels of this lane: 4, or 1 - 3 at the end of a row
  for (int y = blockIdx.y; y < p.drows; y += gridDim.y) {
    const float* m = p.map_xy + ((size_t)y * (size_t)p.dcols + (size_t)x0) * 2;
    float mx[kMaskPxPerLane], my[kMaskPxPerLane];
    if (n == kMaskPxPerLane && (reinterpret_cast<uintptr_t>(m) & 15) == 0) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(m), b = *reinterpret_cast<const f32x4*>(m + 4);
      mx[0] = a.x; my[0] = a.y; mx[1] = a.z; my[1] = a.w;
      mx[2] = b.x; my[2] = b.y; mx[3] = b.z; my[3] = b.w;
    } else {
#pragma unroll
      for (int j = 0; j < kMaskPxPerLane; j++) {
        f32x2 e = {0.f, 0.f};
        if (j < n) e = *reinterpret_cast<const f32x2*>(m + 2 * j);
        mx[j] = e.x;
        my[j] = e.y;
      }
    }
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < kMaskPxPerLane; j++) v |= mask_value<BINARY>(mx[j], my[j], p.src_rows, p.src_cols) << (8 * j);
    uint8_t* row = p.dst + (size_t)y * p.dst_step;
    uint8_t* q = row + x0;
    if (n == kMaskPxPerLane && (reinterpret_cast<uintptr_t>(row) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(q) = v;
    } else {
      for (int j = 0; j < n; j++) q[j] = (uint8_t)(v >> (8 * j));
    }
  }
}

__global__ __launch_bounds__(kMaskBlock) void mask_threshold_kernel(MaskThresholdParams p) {
  const int x0 = ((int)blockIdx.x * kMaskBlock + (int)threadIdx.x) * kMaskPxPerLane;
  if (x0 >= p.cols) return;
  for (int y = blockIdx.y; y < p.rows; y += gridDim.y) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p.img + (size_t)y * p.step + x0);
    const uint32_t v = *q;
    uint32_t o = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) o |= (((v >> (8 * j)) & 255u) == 255u ? 255u : 0u) << (8 * j);
    *q = o;
  }
}

bool launch_rect_mask(const RectMaskParams& p, hipStream_t stream, LaunchInfo* info) {
  if (!p.map_xy || !p.dst || p.drows < 1 || p.dcols < 1 || p.src_rows < 1 || p.src_cols < 1) return false;
  if (reinterpret_cast<uintptr_t>(p.map_xy) & 7) return false;
  if (p.dst_step < (size_t)p.dcols) return false;
  const dim3 grid((unsigned)((p.dcols + kMaskPxPerBlock - 1) / kMaskPxPerBlock), (unsigned)(p.drows < 65535 ? p.drows : 65535));
  if (p.binary) hipLaunchKernelGGL(rect_mask_kernel<true>, grid, dim3(kMaskBlock), 0, stream, p);
  else hipLaunchKernelGGL(rect_mask_kernel<false>, grid, dim3(kMaskBlock), 0, stream, p);
  if (info) *info = LaunchInfo{p.binary ? "rect_mask_kernel<true>" : "rect_mask_kernel<false>", grid.x, grid.y, (unsigned)kMaskBlock};
  return true;
}

bool launch_mask_threshold(const MaskThresholdParams& p, hipStream_t stream, LaunchInfo* info) {
  if (!p.img || p.rows < 1 || p.cols < 1) return false;
  if ((reinterpret_cast<uintptr_t>(p.img) | p.step) & 3) return false;
  if (p.step < (((size_t)p.cols + 3) & ~(size_t)3)) return false;
  const dim3 grid((unsigned)((p.cols + kMaskPxPerBlock - 1) / kMaskPxPerBlock), (unsigned)(p.rows < 65535 ? p.rows : 65535));
  hipLaunchKernelGGL(mask_threshold_kernel, grid, dim3(kMaskBlock), 0, stream, p);
  if (info) *info = LaunchInfo{"mask_threshold_kernel", grid.x, grid.y, (unsigned)kMaskBlock};
  return true;
}

}  // namespace rip
