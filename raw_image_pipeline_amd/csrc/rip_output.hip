// rip_output.hip -- the output stage (rip_set_output_format, rip_output.hpp): the pipeline's final interleaved BGR image ->
// rgb8 / mono8 / normalised planar float tensors, one launch per batch slice.  Built into librip_out_hip.so.
//
// A lane owns 4 consecutive pixels of one row: it reads their 12 bytes as three dwords (source rows are 4-byte aligned) and
// writes, per plane, one store of 4 elements -- 16 B (f32), 8 B (f16 / bf16), 12 B (rgb8) or 4 B (mono8).  A workgroup of 256
// lanes covers 1024 pixels of one row; every channel value is a byte, so a planar element is one entry of a 3 x 256 table
// (built on the host, rip::build_output_table) that each workgroup copies into LDS once.
//
// The destination is the caller's: a wide store is used only where the first element of the row (and plane) is aligned to the
// store's width -- the lanes of a row start whole stores apart, so the test is per row and wave-uniform -- and single elements
// otherwise; the last lane of a row writes the 1 - 3 pixels that are left as single elements.  Nothing is written at or beyond
// column `cols` of any row.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rip_output.hpp"

namespace rip {
namespace {
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// the formats: element type (f16 / bf16 travel as their bit patterns), planar or interleaved, plane order
struct Rgb8 { using elem = uint8_t; static constexpr bool planar = false, rgb = true; };
struct Mono8 { using elem = uint8_t; static constexpr bool planar = false, rgb = false; };
struct RgbChwF32 { using elem = uint32_t; static constexpr bool planar = true, rgb = true; };
struct RgbChwF16 { using elem = uint16_t; static constexpr bool planar = true, rgb = true; };
struct RgbChwBf16 { using elem = uint16_t; static constexpr bool planar = true, rgb = true; };
struct BgrChwF32 { using elem = uint32_t; static constexpr bool planar = true, rgb = false; };
struct BgrChwF16 { using elem = uint16_t; static constexpr bool planar = true, rgb = false; };
struct BgrChwBf16 { using elem = uint16_t; static constexpr bool planar = true, rgb = false; };

// 4 elements at q: one wide store when `wide` (q is then aligned to 4 elements) and all 4 are wanted, else n single elements
__device__ __forceinline__ void store4(uint32_t* q, const uint32_t v[4], int n, bool wide) {
  if (wide && n == 4) {
    *reinterpret_cast<u32x4*>(q) = u32x4{v[0], v[1], v[2], v[3]};
  } else {
    for (int j = 0; j < n; j++) q[j] = v[j];
  }
}
__device__ __forceinline__ void store4(uint16_t* q, const uint16_t v[4], int n, bool wide) {
  if (wide && n == 4) {
    *reinterpret_cast<u32x2*>(q) = u32x2{(uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16)};
  } else {
    for (int j = 0; j < n; j++) q[j] = v[j];
  }
}
__device__ __forceinline__ void store4(uint8_t* q, const uint8_t v[4], int n, bool wide) {
  if (wide && n == 4) {
    *reinterpret_cast<uint32_t*>(q) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
  } else {
    for (int j = 0; j < n; j++) q[j] = v[j];
  }
}

template <typename Fmt>
__global__ __launch_bounds__(kOutBlock) void output_convert_kernel(OutputConvertParams p) {
  using E = typename Fmt::elem;
  __shared__ E tab[Fmt::planar ? 768 : 1];
  if constexpr (Fmt::planar) {
    const E* t = static_cast<const E*>(p.table);
    for (int i = threadIdx.x; i < 768; i += kOutBlock) tab[i] = t[i];
    __syncthreads();
  }
  const int x0 = ((int)blockIdx.x * kOutBlock + (int)threadIdx.x) * kOutPxPerLane;
  if (x0 >= p.cols) return;
  const int n = min(kOutPxPerLane, p.cols - x0);  // pixels of this lane: 4, or 1 - 3 at the end of a row
  const uint8_t* src_frame = p.src + (size_t)blockIdx.z * p.src_frame_stride;
  uint8_t* dst_frame = static_cast<uint8_t*>(p.dst) + (size_t)blockIdx.z * p.dst_frame_stride;
  for (int y = blockIdx.y; y < p.rows; y += gridDim.y) {
    // the dwords that hold a byte of the lane's pixels; rows are 4-byte aligned and src_step bytes long, so each lies inside the row
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src_frame + (size_t)y * p.src_step + (size_t)x0 * 3);
    uint32_t w[3];
#pragma unroll
    for (int k = 0; k < 3; k++) w[k] = 4 * k < 3 * n ? s[k] : 0u;
    uint8_t b[12];  // B G R of the lane's pixels
#pragma unroll
    for (int i = 0; i < 12; i++) b[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    if constexpr (Fmt::planar) {
      const size_t plane = p.dst_step * (size_t)p.rows;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        uint8_t* row = dst_frame + (size_t)c * plane + (size_t)y * p.dst_step;
        const bool wide = (reinterpret_cast<uintptr_t>(row) & (4 * sizeof(E) - 1)) == 0;
        const int ch = Fmt::rgb ? 2 - c : c;
        E v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = tab[c * 256 + b[3 * j + ch]];
        store4(reinterpret_cast<E*>(row) + x0, v, n, wide);
      }
    } else if constexpr (Fmt::rgb) {  // rgb8: the channels of every pixel reversed, 12 bytes per lane
      uint8_t* row = dst_frame + (size_t)y * p.dst_step;
      uint8_t* q = row + (size_t)x0 * 3;
      if ((reinterpret_cast<uintptr_t>(row) & 3) == 0 && n == 4) {
        uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 12; i++) o[i >> 2] |= (uint32_t)b[i - i % 3 + 2 - i % 3] << (8 * (i & 3));
        uint32_t* q4 = reinterpret_cast<uint32_t*>(q);
        q4[0] = o[0];
        q4[1] = o[1];
        q4[2] = o[2];
      } else {
        for (int j = 0; j < n; j++) {
          q[3 * j] = b[3 * j + 2];
          q[3 * j + 1] = b[3 * j + 1];
          q[3 * j + 2] = b[3 * j];
        }
      }
    } else {  // mono8: (3735 B + 19235 G + 9798 R + 16384) >> 15
      uint8_t* row = dst_frame + (size_t)y * p.dst_step;
      uint8_t v[4];
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = (uint8_t)((3735u * b[3 * j] + 19235u * b[3 * j + 1] + 9798u * b[3 * j + 2] + 16384u) >> 15);
      store4(row + x0, v, n, (reinterpret_cast<uintptr_t>(row) & 3) == 0);
    }
  }
}

template <typename Fmt>
void launch(const OutputConvertParams& p, hipStream_t stream, const char* name, LaunchInfo* info) {
  const dim3 grid((unsigned)((p.cols + kOutPxPerBlock - 1) / kOutPxPerBlock), (unsigned)(p.rows < 65535 ? p.rows : 65535), (unsigned)p.n_frames);
  hipLaunchKernelGGL(output_convert_kernel<Fmt>, grid, dim3(kOutBlock), 0, stream, p);
  if (info) *info = LaunchInfo{name, grid.x, grid.y, (unsigned)kOutBlock};
}
}  // namespace

bool launch_output_convert(const OutputConvertParams& p, hipStream_t stream, LaunchInfo* info) {
  if (!p.src || !p.dst || p.rows < 1 || p.cols < 1 || p.n_frames < 1 || p.n_frames > 65535) return false;
  if ((reinterpret_cast<uintptr_t>(p.src) | p.src_step | p.src_frame_stride) & 3) return false;
  if (p.src_step < (((size_t)p.cols * 3 + 3) & ~(size_t)3)) return false;
  const size_t e = (size_t)output_format_elem_bytes(p.format);
  if (output_format_planar(p.format) && (!p.table || (reinterpret_cast<uintptr_t>(p.dst) | p.dst_step | p.dst_frame_stride) % e != 0)) return false;
  if (p.dst_step < (size_t)p.cols * e * (output_format_planar(p.format) ? 1 : output_format_channels(p.format))) return false;
  switch (p.format) {
    case OUT_RGB8: launch<Rgb8>(p, stream, "output_convert_kernel<Rgb8>", info); return true;
    case OUT_MONO8: launch<Mono8>(p, stream, "output_convert_kernel<Mono8>", info); return true;
    case OUT_RGB_CHW_F32: launch<RgbChwF32>(p, stream, "output_convert_kernel<RgbChwF32>", info); return true;
    case OUT_RGB_CHW_F16: launch<RgbChwF16>(p, stream, "output_convert_kernel<RgbChwF16>", info); return true;
    case OUT_RGB_CHW_BF16: launch<RgbChwBf16>(p, stream, "output_convert_kernel<RgbChwBf16>", info); return true;
    case OUT_BGR_CHW_F32: launch<BgrChwF32>(p, stream, "output_convert_kernel<BgrChwF32>", info); return true;
    case OUT_BGR_CHW_F16: launch<BgrChwF16>(p, stream, "output_convert_kernel<BgrChwF16>", info); return true;
    case OUT_BGR_CHW_BF16: launch<BgrChwBf16>(p, stream, "output_convert_kernel<BgrChwBf16>", info); return true;
    default: return false;
  }
}

}  // namespace rip
