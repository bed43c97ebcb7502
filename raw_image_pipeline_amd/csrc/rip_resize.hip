// rip_resize.hip -- the resize stage (rip_set_output_size, rip_resize.hpp): cv::resize(F, size, INTER_LINEAR) on the pipeline's final
// 8-bit image of 1 or 3 interleaved channels, one launch per batch slice.  Built into librip_rsz_hip.so.
//
// A lane owns 4 consecutive output pixels of one row, a workgroup of 256 lanes covers 1024 of them; the grid's y walks the output
// rows.  Everything that depends on the column alone -- byte offset of the first tap, whether a second tap exists, the two
// weights -- is read from the per-column tables once, in front of the row loop; the per-row tables give the two source rows and
// their weights.  The kernel does integer work only (PARITY.md "Resize"):
//   h_k = S_k[sx] * a0 + S_k[sx'] * a1 for the rows k = 0, 1;  value = (((b0 * (h_0 >> 4)) >> 16) + ((b1 * (h_1 >> 4)) >> 16) + 2) >> 2
// and, when the source is exactly twice the target on both axes, the mean (a + b + c + d + 2) >> 2 of every 2 x 2 block.
//
// Source rows are 4-byte aligned: the two taps of a pixel are 2 or 6 adjacent bytes, read as the two or three aligned dwords that
// hold them (a dword index beyond the row's last dword is clamped to it: it can only hold a second tap that does not exist).  The
// destination is the caller's: dword stores only where the row start is 4-byte aligned (the lanes of a row start whole stores
// apart, so the test is per row and wave-uniform), single bytes otherwise and for the 1 - 3 pixels at a row's end.  Nothing is
// written at or beyond column `cols` of any row.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rip_resize.hpp"

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

template <int CH, bool AREA>
__global__ __launch_bounds__(kRszBlock) void resize_kernel(ResizeParams p) {
  const int x0 = ((int)blockIdx.x * kRszBlock + (int)threadIdx.x) * kRszPxPerLane;
  if (x0 >= p.cols) return;
  const int n = min(kRszPxPerLane, p.cols - x0);  // pixels of this lane: 4, or 1 - 3 at the end of a row
  const uint8_t* src_frame = p.src + (size_t)blockIdx.z * p.src_frame_stride;
  uint8_t* dst_frame = p.dst + (size_t)blockIdx.z * p.dst_frame_stride;
  uint8_t v[4 * CH];
#pragma unroll
  for (int i = 0; i < 4 * CH; i++) v[i] = 0;
  if constexpr (AREA) {
    // the lane's 4 pixels are the means of 8 consecutive source pixels of two rows: 8 * CH bytes from an 8-byte aligned offset
    constexpr int kDw = 2 * CH;
    const int need = (2 * n * CH + 3) >> 2;  // dwords that hold a byte of the lane's source pixels
    for (int y = blockIdx.y; y < p.rows; y += gridDim.y) {
      const uint8_t* s = src_frame + (size_t)(2 * y) * p.src_step + (size_t)x0 * 2 * CH;
      const uint32_t* r0 = reinterpret_cast<const uint32_t*>(s);
      const uint32_t* r1 = reinterpret_cast<const uint32_t*>(s + p.src_step);
      uint32_t w0[kDw], w1[kDw];
#pragma unroll
      for (int k = 0; k < kDw; k++) {
        w0[k] = k < need ? r0[k] : 0u;
        w1[k] = k < need ? r1[k] : 0u;
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
  } else {
    // per column, once: the tables are padded to whole lanes and 16-byte aligned (rip_resize.hpp)
    const i32x4 xo = *reinterpret_cast<const i32x4*>(p.xofs + x0);
    const u32x4 al = *reinterpret_cast<const u32x4*>(p.alpha + 2 * x0);  // (a0, a1) of a pixel in one dword
    int off[4], a0[4], a1[4];
    bool two[4];  // a second tap exists: sx + 1 <= C - 1 (else it is the first tap again)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int sx = xo[j];
      off[j] = sx * CH;
      two[j] = sx + 1 < p.src_cols;
      a0[j] = (int)(int16_t)(al[j] & 0xFFFFu);
      a1[j] = (int)(int16_t)(al[j] >> 16);
    }
    const int last_dw = ((p.src_cols * CH + 3) >> 2) - 1;
    for (int y = blockIdx.y; y < p.rows; y += gridDim.y) {
      const int sy0 = p.yofs[2 * y], sy1 = p.yofs[2 * y + 1];
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
}

template <int CH, bool AREA>
void launch(const ResizeParams& p, hipStream_t stream, const char* name, ResizeLaunchInfo* info) {
  const dim3 grid((unsigned)((p.cols + kRszPxPerBlock - 1) / kRszPxPerBlock), (unsigned)(p.rows < 65535 ? p.rows : 65535), (unsigned)p.n_frames);
  hipLaunchKernelGGL((resize_kernel<CH, AREA>), grid, dim3(kRszBlock), 0, stream, p);
  if (info) *info = ResizeLaunchInfo{name, grid.x, grid.y, (unsigned)kRszBlock};
}
}  // namespace

bool launch_resize(const ResizeParams& p, hipStream_t stream, ResizeLaunchInfo* info) {
  if (!p.src || !p.dst || p.n_frames < 1 || p.n_frames > 65535 || (p.channels != 1 && p.channels != 3)) return false;
  for (int side : {p.src_rows, p.src_cols, p.rows, p.cols})
    if (side < 1 || side > kRszMaxSide) return false;
  if ((reinterpret_cast<uintptr_t>(p.src) | p.src_step | p.src_frame_stride) & 3) return false;
  if (p.src_step < (((size_t)p.src_cols * p.channels + 3) & ~(size_t)3) || p.src_frame_stride < p.src_step * (size_t)p.src_rows) return false;
  if (p.dst_step < (size_t)p.cols * p.channels) return false;
  const bool area = p.src_rows == 2 * p.rows && p.src_cols == 2 * p.cols;
  if (area != (p.area2 != 0)) return false;
  if (!area && (!p.xofs || !p.alpha || !p.yofs || !p.beta || ((reinterpret_cast<uintptr_t>(p.xofs) | reinterpret_cast<uintptr_t>(p.alpha)) & 15) ||
                (reinterpret_cast<uintptr_t>(p.yofs) & 3) || (reinterpret_cast<uintptr_t>(p.beta) & 1)))
    return false;
  if (p.channels == 1) {
    if (area) launch<1, true>(p, stream, "resize_kernel<1, true>", info);
    else launch<1, false>(p, stream, "resize_kernel<1, false>", info);
  } else {
    if (area) launch<3, true>(p, stream, "resize_kernel<3, true>", info);
    else launch<3, false>(p, stream, "resize_kernel<3, false>", info);
  }
  return true;
}

}  // namespace rip
