// rip_heads.hip -- output heads (rip_heads.hpp): rows x row_bytes x frames from the 16-byte aligned staging image to a destination
// of any alignment and pitch, one launch per batch slice.  Built into librip_heads_hip.so.
//
// A lane owns 16 consecutive source bytes of one row and reads them with one 16-byte load (source rows start 16-byte aligned and
// their pitch holds whole 16-byte blocks).  The destination is the caller's: a 16-byte store is used where the first byte of the row
// is 16-byte aligned, four dword stores where it is 4-byte aligned -- the lanes of a row start whole blocks apart, so the test is per
// row and wave-uniform -- and single bytes otherwise; the last lane of a row writes the 1 - 15 bytes that are left as single bytes.
// Nothing is written at or beyond row_bytes of any row.  No LDS, integer moves only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rip_heads.hpp"

namespace rip {
namespace {
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
}

__global__ __launch_bounds__(kHeadBlock) void head_copy_kernel(HeadCopyParams p) {
  const size_t x0 = ((size_t)blockIdx.x * kHeadBlock + threadIdx.x) * kHeadBytesPerLane;
  if (x0 >= p.row_bytes) return;
  const int n = (int)min((size_t)kHeadBytesPerLane, p.row_bytes - x0);  // bytes of this lane: 16, or 1 - 15 at the end of a row
  const uint8_t* src_frame = p.src + (size_t)blockIdx.z * p.src_frame_stride;
  uint8_t* dst_frame = p.dst + (size_t)blockIdx.z * p.dst_frame_stride;
  for (int y = blockIdx.y; y < p.rows; y += gridDim.y) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(src_frame + (size_t)y * p.src_step + x0);
    uint8_t* row = dst_frame + (size_t)y * p.dst_step;
    uint8_t* q = row + x0;
    const unsigned phase = (unsigned)(reinterpret_cast<uintptr_t>(row) & 15);
    if (n == kHeadBytesPerLane && phase == 0) {
      *reinterpret_cast<u32x4*>(q) = v;
    } else if (n == kHeadBytesPerLane && (phase & 3) == 0) {
      uint32_t* q4 = reinterpret_cast<uint32_t*>(q);
      q4[0] = v.x;
      q4[1] = v.y;
      q4[2] = v.z;
      q4[3] = v.w;
    } else {
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < kHeadBytesPerLane; i++)
        if (i < n) q[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
  }
}

bool launch_head_copy(const HeadCopyParams& p, hipStream_t stream, LaunchInfo* info) {
  if (!p.src || !p.dst || p.rows < 1 || p.row_bytes < 1 || p.row_bytes >= ((size_t)1 << 24) || p.n_frames < 1 || p.n_frames > 65535) return false;
  if ((reinterpret_cast<uintptr_t>(p.src) | p.src_step | p.src_frame_stride) & 15) return false;
  if (p.src_step < ((p.row_bytes + 15) & ~(size_t)15) || p.dst_step < p.row_bytes) return false;
  if (p.n_frames > 1 && (p.src_frame_stride < p.src_step * (size_t)p.rows || p.dst_frame_stride < p.dst_step * (size_t)(p.rows - 1) + p.row_bytes)) return false;
  const dim3 grid((unsigned)((p.row_bytes + kHeadBytesPerBlock - 1) / kHeadBytesPerBlock), (unsigned)(p.rows < 65535 ? p.rows : 65535), (unsigned)p.n_frames);
  hipLaunchKernelGGL(head_copy_kernel, grid, dim3(kHeadBlock), 0, stream, p);
  if (info) *info = LaunchInfo{"head_copy_kernel", grid.x, grid.y, (unsigned)kHeadBlock};
  return true;
}

}  // namespace rip
