// rip_yuv.hip -- the YUV 4:2:0 output formats (rip_set_output_format "nv12" / "i420", rip_yuv.hpp): the delivered interleaved BGR
// picture -> a Y plane and 2 x 2 subsampled Cb / Cr, one launch per batch slice.  Built into librip_yuv_hip.so.
//
// A memory-rate pass, 3 B/px read and 1.5 B/px written.  A lane owns 2 rows x 8 columns, four 2 x 2 blocks: it reads the 24 bytes of
// each of its two rows as six dwords (source rows are 4-byte aligned; neighbouring lanes read neighbouring 24 bytes), writes 8 bytes of
// Y per row and 8 bytes of interleaved chroma (nv12) or 4 bytes each of Cb and Cr (i420).  A workgroup of 256 lanes is 64 lanes -- 512
// columns -- wide and 4 row pairs high, so a wave's accesses of one row are contiguous.  All integer: the twelve weights and the Y
// offset travel in the parameter struct.
//
// The destination is the caller's: a wide store is used only where the start of the row is aligned to the store's width -- the lanes
// of a row start whole stores apart, so the test is per row and wave-uniform -- and single bytes otherwise; the last lane of a row whose
// width is no multiple of 8 writes its 2, 4 or 6 columns as single bytes.  Nothing is written at or beyond column `cols` of a Y or nv12
// chroma row, or cols / 2 of an i420 chroma row.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rip_yuv.hpp"

namespace rip {
namespace {
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pack4(const uint8_t* v) {
  return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
}

template <bool SemiPlanar>
__global__ __launch_bounds__(kYuvBlock) void yuv420_kernel(Yuv420Params p) {
  const int lx = (int)threadIdx.x % kYuvLanesX, ly = (int)threadIdx.x / kYuvLanesX;
  const int x0 = ((int)blockIdx.x * kYuvLanesX + lx) * kYuvPxPerLane;
  if (x0 >= p.cols) return;
  const int n = min(kYuvPxPerLane, p.cols - x0);  // columns of this lane: 8, or 2, 4, 6 at the end of a row (cols is even)
  const int pairs = p.rows >> 1;
  const uint8_t* src_frame = p.src + (size_t)blockIdx.z * p.src_frame_stride;
  uint8_t* dst_frame = p.dst + (size_t)blockIdx.z * p.dst_frame_stride;
  const int ybias = (p.m.yoff << 15) + 16384, cbias = (128 << 17) + 65536;
  for (int j = (int)blockIdx.y * kYuvPairsPerBlock + ly; j < pairs; j += (int)gridDim.y * kYuvPairsPerBlock) {
    int sb[4] = {0, 0, 0, 0}, sg[4] = {0, 0, 0, 0}, sr[4] = {0, 0, 0, 0};  // the channel sums of the lane's four 2 x 2 blocks
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int y = 2 * j + r;
      // the dwords that hold a byte of the lane's pixels; rows are 4-byte aligned and src_step bytes long, so each lies inside the row
      const uint32_t* s = reinterpret_cast<const uint32_t*>(src_frame + (size_t)y * p.src_step + (size_t)x0 * 3);
      uint32_t w[6];
#pragma unroll
      for (int k = 0; k < 6; k++) w[k] = 4 * k < 3 * n ? s[k] : 0u;
      uint8_t yv[8];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int b = (int)((w[(3 * i) >> 2] >> (8 * ((3 * i) & 3))) & 255u);
        const int g = (int)((w[(3 * i + 1) >> 2] >> (8 * ((3 * i + 1) & 3))) & 255u);
        const int c = (int)((w[(3 * i + 2) >> 2] >> (8 * ((3 * i + 2) & 3))) & 255u);
        yv[i] = (uint8_t)((p.m.y[0] * b + p.m.y[1] * g + p.m.y[2] * c + ybias) >> 15);
        sb[i >> 1] += b;
        sg[i >> 1] += g;
        sr[i >> 1] += c;
      }
      uint8_t* row = dst_frame + (size_t)y * p.dst_step;
      uint8_t* q = row + x0;
      if (n == 8 && (reinterpret_cast<uintptr_t>(row) & 3) == 0) {
        uint32_t* q4 = reinterpret_cast<uint32_t*>(q);
        q4[0] = pack4(yv);
        q4[1] = pack4(yv + 4);
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++)  // fixed bounds: a loop over n would index the registers dynamically, which means scratch
          if (i < n) q[i] = yv[i];
      }
    }
    uint8_t cb[4], cr[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      cb[i] = (uint8_t)min(255, (p.m.cb[0] * sb[i] + p.m.cb[1] * sg[i] + p.m.cb[2] * sr[i] + cbias) >> 17);
      cr[i] = (uint8_t)min(255, (p.m.cr[0] * sb[i] + p.m.cr[1] * sg[i] + p.m.cr[2] * sr[i] + cbias) >> 17);
    }
    if constexpr (SemiPlanar) {  // Cb Cr of block i at bytes 2 i, 2 i + 1 of the chroma row
      uint8_t* row = dst_frame + (size_t)(p.rows + j) * p.dst_step;
      uint8_t* q = row + x0;
      const uint8_t lo[4] = {cb[0], cr[0], cb[1], cr[1]}, hi[4] = {cb[2], cr[2], cb[3], cr[3]};
      if (n == 8 && (reinterpret_cast<uintptr_t>(row) & 7) == 0) {
        *reinterpret_cast<u32x2*>(q) = u32x2{pack4(lo), pack4(hi)};
      } else if (n == 8 && (reinterpret_cast<uintptr_t>(row) & 3) == 0) {
        uint32_t* q4 = reinterpret_cast<uint32_t*>(q);
        q4[0] = pack4(lo);
        q4[1] = pack4(hi);
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (2 * i < n) {
            q[2 * i] = cb[i];
            q[2 * i + 1] = cr[i];
          }
      }
    } else {  // two planes of rows / 2 rows, half a pitch apart
      const size_t half = p.dst_step >> 1;
      uint8_t* row_cb = dst_frame + (size_t)p.rows * p.dst_step + (size_t)j * half;
      uint8_t* row_cr = row_cb + (size_t)pairs * half;
      uint8_t* qb = row_cb + x0 / 2;
      uint8_t* qr = row_cr + x0 / 2;
      if (n == 8 && (reinterpret_cast<uintptr_t>(row_cb) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(qb) = pack4(cb);
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (2 * i < n) qb[i] = cb[i];
      }
      if (n == 8 && (reinterpret_cast<uintptr_t>(row_cr) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(qr) = pack4(cr);
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (2 * i < n) qr[i] = cr[i];
      }
    }
  }
}

template <bool SemiPlanar>
void launch(const Yuv420Params& p, hipStream_t stream, const char* name, LaunchInfo* info) {
  const int groups = (p.rows / 2 + kYuvPairsPerBlock - 1) / kYuvPairsPerBlock;
  const dim3 grid((unsigned)((p.cols + kYuvPxPerBlockX - 1) / kYuvPxPerBlockX), (unsigned)(groups < 65535 ? groups : 65535), (unsigned)p.n_frames);
  hipLaunchKernelGGL(yuv420_kernel<SemiPlanar>, grid, dim3(kYuvBlock), 0, stream, p);
  if (info) *info = LaunchInfo{name, grid.x, grid.y, (unsigned)kYuvBlock};
}
}  // namespace

bool launch_yuv420(const Yuv420Params& p, hipStream_t stream, LaunchInfo* info) {
  if (!p.src || !p.dst || p.rows < 2 || p.cols < 2 || ((p.rows | p.cols) & 1) || p.n_frames < 1 || p.n_frames > 65535) return false;
  if ((reinterpret_cast<uintptr_t>(p.src) | p.src_step | p.src_frame_stride) & 3) return false;
  if (p.src_step < (((size_t)p.cols * 3 + 3) & ~(size_t)3)) return false;
  if (p.dst_step < (size_t)p.cols || (!p.semi_planar && (p.dst_step & 1))) return false;
  if (p.semi_planar) launch<true>(p, stream, "yuv420_kernel<true>", info);
  else launch<false>(p, stream, "yuv420_kernel<false>", info);
  return true;
}

}  // namespace rip
