// rip_demosaic.hip -- Malvar-He-Cutler demosaic (rip_set_debayer_method "mht"; what the reference's CUDA path computes with
// cv::cuda::demosaicing(..., COLOR_Bayer**2BGR_MHT), debayer.cpp:93-108), with the flip of flip.cpp:40-52 folded into the store.
//
// Contract (PARITY.md): at a site of Bayer phase (dy, dx) = ((y - ry) & 1, (x - rx) & 1) the colour it samples passes
// through; each missing colour is one of four 5 x 5 integer filters of divisor 16 (K_G, K_row, K_col, K_diag below),
// rounded half to even -- (S + 7 + ((S >> 4) & 1)) >> 4 -- and clamped to [0, max].  Reads outside the frame use reflect-101
// (-1 -> 1, -2 -> 2, W -> W - 2, W + 1 -> W - 3), which keeps the Bayer phase.  Output: interleaved BGR of the sample type.
//
// Two kernels:
//   demosaic_mht_tile_kernel   8-bit samples, every flip.  A workgroup stages a 64 x 32 tile plus a 2-px halo in LDS
//                              (2.7 KB; only tiles that touch a frame edge run the reflect-101 index mapping), then each lane
//                              computes an item of 2 rows x 4 px -- every site class, so no lane diverges -- in packed 16-bit
//                              integer arithmetic: pixels j and j + 2 of a row share a site class and ride in the two halves of
//                              one register, so every v_pk_* instruction yields two outputs.  8-bit sums lie in [-3060, 7140].
//                              Flips 0 / 180: 12 B per lane and row stored as three dwords straight from the registers.  Quarter
//                              turns: the BGR tile goes through LDS (6 KB) and is stored transposed, 32-px rows of the rotated
//                              image, 12 B per lane.  The workgroup then moves on to the same tile of the next frame, whose
//                              interior tiles it has been loading into registers meanwhile.  Tiles are dealt to the XCDs in
//                              contiguous ranges (workgroup b runs on XCD b % 8): neighbouring tiles, which share the halo
//                              rows and the cache lines at their seams, are computed by the same XCD.
//   demosaic_mht_pixel_kernel  one thread per destination pixel, 32-bit sums: 16-bit samples (rip_set_debayer_16bit).
#include "rip_kernels.hpp"

#include <algorithm>

namespace rip {
namespace {

constexpr int kMhtBlock = 256;
constexpr int kTileW = 64, kTileH = 32;                   // pixels per tile: 16 x 16 lanes of 4 x 2 items
constexpr int kLdsRows = kTileH + 4;                      // 2-row halo above and below
constexpr int kLdsDwords = (kTileW + 8) / 4;              // columns tx0 - 4 .. tx0 + kTileW + 3: dword-aligned 2-px halo
constexpr int kLdsStride = kLdsDwords + 1;                // dwords per LDS row (odd: lanes of neighbouring rows fall in other banks)
constexpr int kFramesPerBlock = 4;
constexpr int kXcds = 8;

// reflect-101 for the 2-px halo; the final clamp only keeps reads of positions no stored pixel uses inside the frame
__device__ __forceinline__ int reflect101(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return min(max(i, 0), n - 1);
}

__device__ __forceinline__ int mht_round(int s, int maxv) { return min(max((s + 7 + ((s >> 4) & 1)) >> 4, 0), maxv); }

typedef short short2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ short2_t as_s2(uint32_t u) { return __builtin_bit_cast(short2_t, u); }
__device__ __forceinline__ uint32_t as_u32(short2_t v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ short2_t splat(short v) { return short2_t{v, v}; }

// round half to even of s / 16, clamped to [0, 255], on both halves
__device__ __forceinline__ short2_t mht_round2(short2_t s) {
  const short2_t q = (s + splat(7) + ((s >> splat(4)) & splat(1))) >> splat(4);
  return __builtin_elementwise_min(__builtin_elementwise_max(q, splat(0)), splat(255));
}

// ------------------------------------------------------------------------------------------------
// 8-bit: LDS tile, 2 x 4 px per lane, packed 16-bit arithmetic.  RY, RX: the R sample's phase (parse_bayer); ANGLE: the flip.
// ------------------------------------------------------------------------------------------------
template <int RY, int RX, int ANGLE>
__global__ __launch_bounds__(kMhtBlock) void demosaic_mht_tile_kernel(MhtParams p) {
  constexpr bool kFlip180 = ANGLE == 180, kQuarter = ANGLE == 90 || ANGLE == 270;
  __shared__ uint32_t lds[kLdsRows * kLdsStride];
  __shared__ uint32_t obuf[kQuarter ? kTileH * kTileW * 3 / 4 : 1];  // quarter turns: the tile's BGR bytes, source layout
  uint8_t* const lds8 = reinterpret_cast<uint8_t*>(lds);
  // contiguous ranges of (frame group, tile) per XCD; the grid is a multiple of 8
  const int tiles_x = (p.cols + kTileW - 1) / kTileW, tiles_y = (p.rows + kTileH - 1) / kTileH;
  const int tiles = tiles_x * tiles_y, groups = p.frame_groups;
  const int per_xcd = (int)(gridDim.x / kXcds);
  const int v = (int)(blockIdx.x % kXcds) * per_xcd + (int)(blockIdx.x / kXcds);
  if (v >= tiles * groups) return;  // whole workgroup: no barrier has been reached
  const int g = v / tiles, t = v - g * tiles;
  const int tx0 = (t % tiles_x) * kTileW, ty0 = (t / tiles_x) * kTileH;
  const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
  const int x0 = tx0 + 4 * lx, y0 = ty0 + 2 * ly;
  // block-uniform: the halo lies inside the frame and the source can be read in aligned dwords
  const bool interior = p.src_aligned4 && tx0 >= 4 && tx0 + kTileW + 4 <= p.cols && ty0 >= 2 && ty0 + kTileH + 2 <= p.rows;
  const bool active = x0 < p.cols && y0 < p.rows;
  const bool full = x0 + 4 <= p.cols && y0 + 2 <= p.rows;
  // flips 0 / 180: destination of the item's first row and the step between its two rows (180: rows and pixels mirrored)
  const int yd0 = kFlip180 ? p.rows - 1 - y0 : y0;
  const long long row_dir = kFlip180 ? -(long long)p.dst_step : (long long)p.dst_step;
  const int xd_first = kFlip180 ? p.cols - 4 - x0 : x0;  // leftmost destination column of a full item
  // interior tiles: the next frame's tile is loaded into registers while this frame is computed and stored (one tile in
  // flight per workgroup was not enough bytes in flight to cover the memory latency)
  constexpr int kPre = (kLdsRows * kLdsDwords + kMhtBlock - 1) / kMhtBlock;
  uint32_t pre[kPre];
  auto load_tile = [&](int fr) {
    const uint8_t* base = p.src + (size_t)fr * p.src_frame_stride + (size_t)(ty0 - 2) * p.src_step + (size_t)(tx0 - 4);
#pragma unroll
    for (int kk = 0; kk < kPre; kk++) {
      const int k = tid + kk * kMhtBlock, r = k / kLdsDwords, c = k - r * kLdsDwords;
      if (k < kLdsRows * kLdsDwords) pre[kk] = *reinterpret_cast<const uint32_t*>(base + (size_t)r * p.src_step + (size_t)c * 4);
    }
  };
  if (interior) load_tile(g);
  for (int f = g; f < p.n_frames; f += groups) {
    const uint8_t* src = p.src + (size_t)f * p.src_frame_stride;
    uint8_t* dst = p.dst + (size_t)f * p.dst_frame_stride;
    if (interior) {
#pragma unroll
      for (int kk = 0; kk < kPre; kk++) {
        const int k = tid + kk * kMhtBlock, r = k / kLdsDwords, c = k - r * kLdsDwords;
        if (k < kLdsRows * kLdsDwords) lds[r * kLdsStride + c] = pre[kk];
      }
    } else {
      for (int k = tid; k < kLdsRows * kLdsDwords * 4; k += kMhtBlock) {
        const int r = k / (kLdsDwords * 4), c = k - r * (kLdsDwords * 4);
        const int y = reflect101(ty0 - 2 + r, p.rows), x = reflect101(tx0 - 4 + c, p.cols);
        lds8[(r * kLdsStride) * 4 + c] = src[(size_t)y * p.src_step + (size_t)x];
      }
    }
    __syncthreads();
    if (interior && f + groups < p.n_frames) load_tile(f + groups);
    if (active) {
      // P[r][k]: rows y0 - 2 + r, pixel pair (x0 - 2 + k, x0 + k) as two 16-bit lanes
      short2_t P[6][6];
#pragma unroll
      for (int r = 0; r < 6; r++) {
        const uint32_t* row = lds + (2 * ly + r) * kLdsStride + lx;
        const uint32_t d0 = row[0], d1 = row[1], d2 = row[2];
        const uint32_t a = __builtin_amdgcn_alignbyte(d1, d0, 2);  // bytes x0 - 2 .. x0 + 1
        const uint32_t b = __builtin_amdgcn_alignbyte(d2, d1, 2);  // bytes x0 + 2 .. x0 + 5
        P[r][0] = as_s2(a & 0x00FF00FFu);
        P[r][1] = as_s2((a >> 8) & 0x00FF00FFu);
        P[r][2] = as_s2(d1 & 0x00FF00FFu);
        P[r][3] = as_s2((d1 >> 8) & 0x00FF00FFu);
        P[r][4] = as_s2(b & 0x00FF00FFu);
        P[r][5] = as_s2((b >> 8) & 0x00FF00FFu);
      }
      // ch[i][j][c]: output row i, pixels (j, j + 2), channel c (0 B, 1 G, 2 R)
      uint32_t ch[2][2][3];
#pragma unroll
      for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const short2_t c = P[i + 2][j + 2];
          const short2_t h1 = P[i + 2][j + 1] + P[i + 2][j + 3], h2 = P[i + 2][j] + P[i + 2][j + 4];
          const short2_t v1 = P[i + 1][j + 2] + P[i + 3][j + 2], v2 = P[i][j + 2] + P[i + 4][j + 2];
          const int dy = (i + RY) & 1, dx = (j + RX) & 1;
          short2_t r, gr, b;
          if (dy == dx) {  // R (0, 0) or B (1, 1) site: K_G and K_diag
            const short2_t d = (P[i + 1][j + 1] + P[i + 1][j + 3]) + (P[i + 3][j + 1] + P[i + 3][j + 3]);
            const short2_t tt = h2 + v2;
            const short2_t gs = c * splat(8) + (h1 + v1) * splat(4) - tt * splat(2);
            const short2_t xs = c * splat(12) + d * splat(4) - tt * splat(3);
            gr = mht_round2(gs);
            r = dy == 0 ? c : mht_round2(xs);
            b = dy == 0 ? mht_round2(xs) : c;
          } else {  // G site: K_row for the colour of the left / right neighbours, K_col for the upper / lower ones
            const short2_t d2 = ((P[i + 1][j + 1] + P[i + 1][j + 3]) + (P[i + 3][j + 1] + P[i + 3][j + 3])) * splat(2);
            const short2_t c10 = c * splat(10) - d2;
            const short2_t rs = c10 + h1 * splat(8) - h2 * splat(2) + v2;
            const short2_t cs = c10 + v1 * splat(8) + h2 - v2 * splat(2);
            gr = c;
            r = dy == 0 ? mht_round2(rs) : mht_round2(cs);  // red row: R left / right
            b = dy == 0 ? mht_round2(cs) : mht_round2(rs);
          }
          ch[i][j][0] = as_u32(b);
          ch[i][j][1] = as_u32(gr);
          ch[i][j][2] = as_u32(r);
        }
      }
#pragma unroll
      for (int i = 0; i < 2; i++) {
        // byte of pixel q (0..3 of the item, left to right in the source), channel c
        auto px = [&](int q, int c) -> uint32_t { return (ch[i][q & 1][c] >> ((q >> 1) * 16)) & 0xFFu; };
        // destination order: mirrored for the 180-degree flip
        auto o = [&](int k) -> uint32_t { const int q = k / 3, c = k - q * 3; return px(kFlip180 ? 3 - q : q, c); };
        if constexpr (kQuarter) {
          uint32_t* w = obuf + ((2 * ly + i) * kTileW + 4 * lx) * 3 / 4;
          w[0] = o(0) | o(1) << 8 | o(2) << 16 | o(3) << 24;
          w[1] = o(4) | o(5) << 8 | o(6) << 16 | o(7) << 24;
          w[2] = o(8) | o(9) << 8 | o(10) << 16 | o(11) << 24;
        } else if (full && p.dst_aligned4) {
          uint32_t* w = reinterpret_cast<uint32_t*>(dst + (long long)yd0 * (long long)p.dst_step + i * row_dir + (long long)xd_first * 3);
          w[0] = o(0) | o(1) << 8 | o(2) << 16 | o(3) << 24;
          w[1] = o(4) | o(5) << 8 | o(6) << 16 | o(7) << 24;
          w[2] = o(8) | o(9) << 8 | o(10) << 16 | o(11) << 24;
        } else if (y0 + i < p.rows) {
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const int x = x0 + q;
            if (x >= p.cols) break;
            const int xd = kFlip180 ? p.cols - 1 - x : x;
            uint8_t* ob = dst + (long long)yd0 * (long long)p.dst_step + i * row_dir + (long long)xd * 3;
            ob[0] = (uint8_t)px(q, 0);
            ob[1] = (uint8_t)px(q, 1);
            ob[2] = (uint8_t)px(q, 2);
          }
        }
      }
    }
    if constexpr (kQuarter) {
      // the rotated tile: destination row per source column x (90: yd = x, 270: yd = cols - 1 - x), 32 destination pixels
      // per row from the tile's source rows (90: xd = rows - 1 - y, 270: xd = y), 4 of them (12 B) per lane and step
      __syncthreads();
      const uint8_t* ob8 = reinterpret_cast<const uint8_t*>(obuf);
      const int xd_lo = ANGLE == 90 ? p.rows - kTileH - ty0 : ty0;  // destination column of the segment's first pixel
      for (int k = tid; k < kTileW * (kTileH / 4); k += kMhtBlock) {
        const int r = k / (kTileH / 4), q4 = (k - r * (kTileH / 4)) * 4;
        const int x = tx0 + r;
        if (x >= p.cols) continue;
        const int yd = ANGLE == 90 ? x : p.cols - 1 - x;
        uint32_t byte[12];
        bool all = true;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int xd = xd_lo + q4 + e;
          const int y = ANGLE == 90 ? p.rows - 1 - xd : xd;  // source row of destination column xd
          const bool ok = xd >= 0 && y >= ty0 && y < ty0 + kTileH && y < p.rows;
          all = all && ok;
          const uint8_t* s = ob8 + ((ok ? y - ty0 : 0) * kTileW + r) * 3;
          byte[3 * e] = s[0];
          byte[3 * e + 1] = s[1];
          byte[3 * e + 2] = s[2];
        }
        uint8_t* drow = dst + (size_t)yd * p.dst_step;
        if (all && p.dst_aligned4) {
          uint32_t* w = reinterpret_cast<uint32_t*>(drow + (size_t)(xd_lo + q4) * 3);
          w[0] = byte[0] | byte[1] << 8 | byte[2] << 16 | byte[3] << 24;
          w[1] = byte[4] | byte[5] << 8 | byte[6] << 16 | byte[7] << 24;
          w[2] = byte[8] | byte[9] << 8 | byte[10] << 16 | byte[11] << 24;
        } else {
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const int xd = xd_lo + q4 + e;
            const int y = ANGLE == 90 ? p.rows - 1 - xd : xd;
            if (xd < 0 || y < ty0 || y >= ty0 + kTileH || y >= p.rows) continue;
            uint8_t* ob = drow + (size_t)xd * 3;
            ob[0] = (uint8_t)byte[3 * e];
            ob[1] = (uint8_t)byte[3 * e + 1];
            ob[2] = (uint8_t)byte[3 * e + 2];
          }
        }
      }
    }
    __syncthreads();  // the next frame's tile overwrites the LDS
  }
}

// ------------------------------------------------------------------------------------------------
// one thread per destination pixel: 16-bit samples
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void unflip_px(int angle, int rows, int cols, int yd, int xd, int& ys, int& xs) {
  // flip.cpp:40-52: 90 = clockwise (cv::rotate ROTATE_90_CLOCKWISE)
  if (angle == 180) {
    ys = rows - 1 - yd;
    xs = cols - 1 - xd;
  } else if (angle == 90) {
    ys = rows - 1 - xd;
    xs = yd;
  } else if (angle == 270) {
    ys = xd;
    xs = cols - 1 - yd;
  } else {
    ys = yd;
    xs = xd;
  }
}

template <typename T>
__global__ __launch_bounds__(kMhtBlock) void demosaic_mht_pixel_kernel(MhtParams p) {
  const int frame = blockIdx.y;
  const uint8_t* src = p.src + (size_t)frame * p.src_frame_stride;
  uint8_t* dst = p.dst + (size_t)frame * p.dst_frame_stride;
  const int maxv = sizeof(T) == 1 ? 255 : 65535;
  const long long npix = (long long)p.drows * p.dcols;
  for (long long i = (long long)blockIdx.x * kMhtBlock + threadIdx.x; i < npix; i += (long long)gridDim.x * kMhtBlock) {
    const int yd = (int)(i / p.dcols), xd = (int)(i - (long long)yd * p.dcols);
    int y, x;
    unflip_px(p.flip_angle, p.rows, p.cols, yd, xd, y, x);
    auto at = [&](int dy, int dx) {
      const int yy = reflect101(y + dy, p.rows), xx = reflect101(x + dx, p.cols);
      return (int)*reinterpret_cast<const T*>(src + (size_t)yy * p.src_step + (size_t)xx * sizeof(T));
    };
    const int c = at(0, 0);
    const int h1 = at(0, -1) + at(0, 1), h2 = at(0, -2) + at(0, 2);
    const int v1 = at(-1, 0) + at(1, 0), v2 = at(-2, 0) + at(2, 0);
    const int d = at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1);
    const int sy = (y - p.bayer_ry) & 1, sx = (x - p.bayer_rx) & 1;
    int r, g, b;
    if (sy == sx) {  // R or B site
      g = mht_round(8 * c + 4 * (h1 + v1) - 2 * (h2 + v2), maxv);
      const int o = mht_round(12 * c + 4 * d - 3 * (h2 + v2), maxv);
      r = sy == 0 ? c : o;
      b = sy == 0 ? o : c;
    } else {  // G site
      const int rs = mht_round(10 * c + 8 * h1 - 2 * h2 + v2 - 2 * d, maxv);
      const int cs = mht_round(10 * c + 8 * v1 + h2 - 2 * v2 - 2 * d, maxv);
      g = c;
      r = sy == 0 ? rs : cs;
      b = sy == 0 ? cs : rs;
    }
    T* o = reinterpret_cast<T*>(dst + (size_t)yd * p.dst_step + (size_t)xd * 3 * sizeof(T));
    o[0] = (T)b;
    o[1] = (T)g;
    o[2] = (T)r;
  }
}

template <int RY, int RX>
void launch_tile(const MhtParams& p, dim3 grid, hipStream_t stream) {
  RIP_LOG_LAUNCH(grid, kMhtBlock, p.n_frames, "demosaic_mht_tile_kernel<%d, %d, %d>", RY, RX, p.flip_angle);
  switch (p.flip_angle) {
    case 90: hipLaunchKernelGGL((demosaic_mht_tile_kernel<RY, RX, 90>), grid, dim3(kMhtBlock), 0, stream, p); break;
    case 180: hipLaunchKernelGGL((demosaic_mht_tile_kernel<RY, RX, 180>), grid, dim3(kMhtBlock), 0, stream, p); break;
    case 270: hipLaunchKernelGGL((demosaic_mht_tile_kernel<RY, RX, 270>), grid, dim3(kMhtBlock), 0, stream, p); break;
    default: hipLaunchKernelGGL((demosaic_mht_tile_kernel<RY, RX, 0>), grid, dim3(kMhtBlock), 0, stream, p); break;
  }
}

bool aligned4p(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 3u) == 0; }

}  // namespace

int mht_uses_tile_path(const MhtParams& p) { return p.elem_bytes == 1 ? 1 : 0; }

void launch_demosaic_mht(const MhtParams& p_in, hipStream_t stream) {
  if (p_in.n_frames <= 0) return;
  MhtParams p = p_in;
  if (mht_uses_tile_path(p)) {
    const int a = p.flip_angle == 90 || p.flip_angle == 180 || p.flip_angle == 270 ? p.flip_angle : 0;
    p.flip_angle = a;
    p.src_aligned4 = aligned4p(p.src) && p.src_step % 4 == 0 && p.src_frame_stride % 4 == 0;
    // 4-aligned dword stores: a quarter turn by 90 starts its 32-px segments at rows - 32 - ty0
    p.dst_aligned4 = aligned4p(p.dst) && p.dst_step % 4 == 0 && p.dst_frame_stride % 4 == 0 && (a != 180 || p.cols % 4 == 0) &&
                     (a != 90 || p.rows % 4 == 0);
    const long long tiles = (long long)((p.cols + kTileW - 1) / kTileW) * ((p.rows + kTileH - 1) / kTileH);
    // kFramesPerBlock frames per workgroup visit; fewer groups (more frames per visit) if the 1-D grid would overflow
    const long long max_groups = std::max(1LL, 0x7fffff00LL / tiles);
    p.frame_groups = (int)std::min<long long>((p.n_frames + kFramesPerBlock - 1) / kFramesPerBlock, max_groups);
    const long long grid = ((tiles * p.frame_groups) + kXcds - 1) / kXcds * kXcds;
    const int phase = p.bayer_ry * 2 + p.bayer_rx;
    if (phase == 0) launch_tile<0, 0>(p, dim3((unsigned)grid), stream);
    else if (phase == 1) launch_tile<0, 1>(p, dim3((unsigned)grid), stream);
    else if (phase == 2) launch_tile<1, 0>(p, dim3((unsigned)grid), stream);
    else launch_tile<1, 1>(p, dim3((unsigned)grid), stream);
    return;
  }
  const long long npix = (long long)p.drows * p.dcols;
  const int blocks = (int)std::max(1LL, std::min(4096LL, (npix + kMhtBlock - 1) / kMhtBlock));
  RIP_LOG_LAUNCH(dim3(blocks, p.n_frames), kMhtBlock, p.n_frames, "demosaic_mht_pixel_kernel<unsigned short>");
  hipLaunchKernelGGL(demosaic_mht_pixel_kernel<uint16_t>, dim3(blocks, p.n_frames), dim3(kMhtBlock), 0, stream, p);
}

}  // namespace rip
