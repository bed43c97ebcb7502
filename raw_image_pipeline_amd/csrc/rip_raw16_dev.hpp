// rip_raw16_dev.hpp -- the kernel behind rip_raw16.hip (bayer_*16 frames with a 16-bit range) and rip_packed.hip (packed 10- /
// 12-bit Bayer frames): demosaic at 16 bits, narrowing to 8 bits and the flip of flip.cpp:40-52 in ONE pass, 3 B/px written.
// Everything behind it sees the result exactly as it would see a bgr8 frame holding it (PARITY.md "16-bit Bayer frames through
// the whole chain", "Packed 10- and 12-bit Bayer frames").  The two files differ in one template argument, the STAGING of the
// LDS tile (StageU16 / StagePacked below): what a sample of the source is and how an interior tile's rows are fetched.
//
// Contract:
//   demosaic   bilinear: the two-tap / four-tap rounding averages of debayer16_kernel (rip_chain.hip; cv::demosaicing's
//              Bayer2RGB_Invoker<ushort>), border rule: the interior formula at the position clamped to [1, n - 2].
//              mht: the four 5 x 5 filters of rip_demosaic.hip on 16-bit samples, rounded half to even, clamped to [0, 65535],
//              reflect-101 reads outside the frame.
//   narrowing  n(v) = min(255, floor((510 * max(v - black, 0) + R) / (2 R))), R = white - black: 255 (v - black) / R rounded half
//              up.  No division in the loop: t = clamp(v - black, 0, R) makes the numerator 510 t + R < 2^26, and for numerators
//              below 2^N the quotient by d is (num * M) >> (N + l) with l = ceil(log2 d), M = ceil(2^(N + l) / d) (Granlund and
//              Montgomery, "Division by invariant integers using multiplication", PLDI 1994, theorem 4.2).  N = 26, d = 2 R:
//              2^26 <= M < 2^27; the numerator is shifted left by 6 so that the quotient is v_mul_hi_u32's result shifted right
//              by l.  The clamp to R also stands in for MHT's clamp to [0, 65535] (black >= 0, black + R <= 65535).
//
// The kernel follows demosaic_mht_tile_kernel (rip_demosaic.hip): a workgroup stages a 64 x 32 tile plus a 2-px halo of uint16
// samples in LDS (36 rows of 34 dwords, odd row stride of 35: 5040 B), interior tiles with aligned dword loads and the next
// frame's tile prefetched into registers, edge tiles sample by sample through reflect-101 (clamped into the frame).  Each lane
// computes an item of 2 rows x 4 px -- every site class, so no lane diverges -- in 32-bit integer arithmetic (bilinear sums reach
// 4 * 65535 + 2, MHT sums lie in [-786 420, 1 834 980]: no packed 16-bit forms).  Bilinear's border rule is not an index mapping
// (the clamped position has another Bayer phase): in the tiles that touch the frame's edge -- a block-uniform branch -- every
// pixel is computed at its clamped position with that position's phase, by selects, from the same LDS tile, whose 2-px halo
// covers the clamped position's neighbourhood.  Stores, frame loop and the deal of the tiles to the XCDs: as in the MHT kernel.
//
// Packed staging.  The same 36 x 68 uint16 tile comes out of packed bytes.  A tile row's span never starts on a dword (at
// tx0 = 64 k sample tx0 - 2 sits at byte 96 k - 3 of a 12-bit row, at bit 640 k - 20 of a 10-bit one), so an interior tile
// loads, per LDS dword (two neighbouring samples: 20 or 24 bits, or two of the four high bytes of a CSI-2 RAW10 group plus its
// fifth byte), the two aligned dwords it lies in, keeps them in registers until the tile of the frame before has been
// consumed -- twice the registers of the uint16 staging (10 instead of 5), no LDS of its own -- and extracts with one funnel
// shift over the two dwords (v_lshrrev_b64) plus masks.  Only dwords that hold a byte of a needed sample are addressed (a pair
// inside the span's last dword takes the two dwords that end there), so the one read beyond a row's payload is the tail of
// the span's last dword: inside the pitch, because an interior tile needs a 4-aligned pitch that covers the row -- and in the
// frame's last row only if the payload itself covers it (the last frame may end with its last row).  Edge tiles, and every
// tile of an unaligned source, go sample by sample through the extract functions of rip_unpack.hpp, which read the one or two
// bytes a sample lies in.
#pragma once

#include "rip_kernels.hpp"
#include "rip_unpack.hpp"

#include <algorithm>
#include <cstdio>

namespace rip {
namespace {

constexpr int kBlock16 = 256;
constexpr int kTileW = 64, kTileH = 32;       // pixels per tile: 16 x 16 lanes of 4 x 2 items
constexpr int kLdsRows = kTileH + 4;          // 2-row halo above and below
constexpr int kLdsDwords = (kTileW + 4) / 2;  // samples tx0 - 2 .. tx0 + kTileW + 1, two per dword (tx0 - 2 is even: dword-aligned)
constexpr int kLdsStride = kLdsDwords + 1;    // dwords per LDS row (odd: lanes of neighbouring rows fall in other banks)
constexpr int kFramesPerBlock = 4;
constexpr int kXcds = 8;

// reflect-101 for the 2-px halo; the final clamp only keeps reads of positions no stored pixel uses inside the frame
__device__ __forceinline__ int reflect101(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return min(max(i, 0), n - 1);
}

// round half to even of s / 16; the clamp to [0, 65535] is the narrowing's
__device__ __forceinline__ int mht_round16(int s) { return (s + 7 + ((s >> 4) & 1)) >> 4; }

struct Narrow {
  int black, range;
  uint32_t mul;
  int shift;
  __device__ __forceinline__ uint32_t operator()(int v) const {
    const int t = min(max(v - black, 0), range);
    const uint32_t num = (uint32_t)t * 510u + (uint32_t)range;
    return __umulhi(num << 6, mul) >> shift;
  }
};

// one pixel by the bilinear formulas with a run-time Bayer phase, from the LDS tile (s16: its samples, row stride 2 * kLdsStride);
// (r, c): the pixel's tile position, 1 <= r, c so that its 3 x 3 neighbourhood is staged.  Selects, no branch: the lanes of an edge
// tile hold every site class.
__device__ __forceinline__ void bilinear_at(const uint16_t* s16, int r, int c, int dy, int dx, int& b, int& g, int& rr) {
  const uint16_t* m = s16 + r * (2 * kLdsStride) + c;
  const uint16_t* u = m - 2 * kLdsStride;
  const uint16_t* d = m + 2 * kLdsStride;
  const int ctr = m[0], hs = (int)m[-1] + (int)m[1], vs = (int)u[0] + (int)d[0];
  const int d4 = ((int)u[-1] + (int)u[1] + (int)d[-1] + (int)d[1] + 2) >> 2;
  const bool green = dy != dx;
  const int own = green ? (hs + 1) >> 1 : ctr;  // the colour of this row's R / B sites
  const int other = green ? (vs + 1) >> 1 : d4;
  g = green ? ctr : (hs + vs + 2) >> 2;
  rr = dy == 0 ? own : other;
  b = dy == 0 ? other : own;
}

// uint16 samples, two per dword: an interior tile's row is kLdsDwords aligned dwords (tx0 - 2 is even)
struct StageU16 {
  static constexpr bool kPacked = false;
  static constexpr int kLayout = 0;
  __device__ static __forceinline__ uint32_t sample(const uint8_t* row, int x) { return *reinterpret_cast<const uint16_t*>(row + (size_t)x * 2); }
};

// packed rows (rip_unpack.hpp).  c: LDS dword of a tile row, samples x = tx0 - 2 + 2 c (even) and x + 1.
template <int LAYOUT>
struct StagePacked {
  static constexpr bool kPacked = true;
  static constexpr int kLayout = LAYOUT;
  static constexpr int kBits = LAYOUT == PACKED_10P || LAYOUT == PACKED_10_CSI2 ? 10 : 12;
  __device__ static __forceinline__ uint32_t sample(const uint8_t* row, int x) { return unpack_sample<LAYOUT>(row, x); }
  // dword of the row that holds the last byte the tile at tx0 needs (sample tx0 + kTileW + 1)
  __device__ static __forceinline__ int last_dword(int tx0) {
    if constexpr (LAYOUT == PACKED_10_CSI2) return (5 * ((tx0 + kTileW + 1) >> 2) + 4) >> 2;
    else return ((tx0 + kTileW + 2) * kBits - 1) >> 5;
  }
  // the dwords lo and lo + 1 of the row the pair lies in, and the shift (0 .. 63) that brings its first bit (CSI-2 RAW10:
  // its group's first byte) to bit 0 of the two read as 64 bits.  12p and CSI-2 RAW12 place a pair in the same three bytes:
  // 12 x / 8 = 3 (x / 2) for even x.  Both dwords hold bytes of the tile's samples: a pair that starts in the span's last
  // dword ends there, and is addressed as the upper of the two before it (shift of 32 and more).  CSI-2 RAW10: a group's
  // first byte lies in lo and its fifth in lo + 1, always, and the shift stays below 32.
  __device__ static __forceinline__ void locate(int tx0, int c, int& lo, int& sh) {
    const int x = tx0 - 2 + 2 * c;
    const int bit = LAYOUT == PACKED_10_CSI2 ? 40 * (x >> 2) : kBits * x;
    lo = bit >> 5;
    sh = bit & 31;
    if constexpr (LAYOUT != PACKED_10_CSI2) {
      const int last = 1 + ((lo - last_dword(tx0)) >> 31);  // 1 in the span's last dword, else 0 (lo never lies beyond it);
      lo -= last;                                           // in arithmetic: a select would keep a lane mask per pair alive
      sh += 32 * last;
    }
  }
  // the LDS dword: sample x in the lower half, x + 1 in the upper
  __device__ static __forceinline__ uint32_t decode(uint32_t dlo, uint32_t dhi, int sh, int x) {
    // the funnel shift over the two dwords
    const uint32_t w = (uint32_t)((((uint64_t)dhi << 32) | dlo) >> sh);
    if constexpr (LAYOUT == PACKED_10P) {
      return (w & 0x3FFu) | ((w << 6) & 0x3FF0000u);
    } else if constexpr (LAYOUT == PACKED_12P) {
      return (w & 0xFFFu) | ((w << 4) & 0xFFF0000u);
    } else if constexpr (LAYOUT == PACKED_12_CSI2) {
      // bytes b0 b1 b2: b0 << 4 | b2 & 15, b1 << 4 | b2 >> 4
      return ((w & 0xFFu) << 4) | ((w >> 16) & 15u) | ((w << 12) & 0xFF00000u) | ((w >> 4) & 0xF0000u);
    } else {
      // bytes b0 .. b3 of the group in w, its fifth byte b4 at the same shift in the upper dword (the group's first byte
      // lies in the lower one, so b4 always lies in the upper); x & 3 is 0 or 2
      const int j = x & 3;
      const uint32_t v = (uint32_t)((((uint64_t)dhi << 32) | dlo) >> (sh + 8 * j)), l = dhi >> (sh + 2 * j);
      return ((v & 0xFFu) << 2) | (l & 3u) | ((v << 10) & 0x3FC0000u) | ((l << 14) & 0x30000u);
    }
  }
};

// L: the staging; MHT: the demosaic method; RY, RX: the R sample's phase (parse_bayer); ANGLE: the flip.
template <class L, bool MHT, int RY, int RX, int ANGLE>
__global__ __launch_bounds__(kBlock16) void raw16_tile_kernel(Raw16Params p) {
  constexpr bool kFlip180 = ANGLE == 180, kQuarter = ANGLE == 90 || ANGLE == 270;
  __shared__ uint32_t lds[kLdsRows * kLdsStride];
  __shared__ uint32_t obuf[kQuarter ? kTileH * kTileW * 3 / 4 : 1];  // quarter turns: the tile's BGR bytes, source layout
  uint16_t* const lds16 = reinterpret_cast<uint16_t*>(lds);
  const Narrow narrow{p.black, p.range, p.mul, p.shift};
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
  bool interior = p.src_aligned4 && tx0 >= 2 && tx0 + kTileW + 2 <= p.cols && ty0 >= 2 && ty0 + kTileH + 2 <= p.rows;
  if constexpr (L::kPacked)  // the tail of the span's last dword: in the pitch, but in the frame's last row only in its payload
    interior = interior && (4 * (size_t)L::last_dword(tx0) + 4 <= (((size_t)p.cols * L::kBits + 7) >> 3) || ty0 + kTileH + 2 < p.rows);
  const bool active = x0 < p.cols && y0 < p.rows;
  const bool full = x0 + 4 <= p.cols && y0 + 2 <= p.rows;
  // flips 0 / 180: destination of the item's first row and the step between its two rows (180: rows and pixels mirrored)
  const int yd0 = kFlip180 ? p.rows - 1 - y0 : y0;
  const long long row_dir = kFlip180 ? -(long long)p.dst_step : (long long)p.dst_step;
  const int xd_first = kFlip180 ? p.cols - 4 - x0 : x0;  // leftmost destination column of a full item
  // interior tiles: the next frame's tile is loaded into registers while this frame is computed and stored
  constexpr int kPre = (kLdsRows * kLdsDwords + kBlock16 - 1) / kBlock16;
  uint32_t pre[kPre];
  uint32_t pre_hi[L::kPacked ? kPre : 1];  // packed: the dword above
  auto load_tile = [&](int fr) {
    if constexpr (L::kPacked) {
      const uint8_t* base = p.src + (size_t)fr * p.src_frame_stride + (size_t)(ty0 - 2) * p.src_step;
#pragma unroll
      for (int kk = 0; kk < kPre; kk++) {
        const int k = tid + kk * kBlock16, r = k / kLdsDwords, c = k - r * kLdsDwords;
        if (k < kLdsRows * kLdsDwords) {
          int lo, sh;
          L::locate(tx0, c, lo, sh);
          // one 32-bit offset per pair (a frame stays below 4 GiB: rip_apply_device), the upper dword 4 bytes on
          const uint32_t* d = reinterpret_cast<const uint32_t*>(base + ((uint32_t)r * (uint32_t)p.src_step + 4u * (uint32_t)lo));
          pre[kk] = d[0];
          pre_hi[kk] = d[1];
        }
      }
    } else {
      const uint8_t* base = p.src + (size_t)fr * p.src_frame_stride + (size_t)(ty0 - 2) * p.src_step + (size_t)(tx0 - 2) * 2;
#pragma unroll
      for (int kk = 0; kk < kPre; kk++) {
        const int k = tid + kk * kBlock16, r = k / kLdsDwords, c = k - r * kLdsDwords;
        if (k < kLdsRows * kLdsDwords) pre[kk] = *reinterpret_cast<const uint32_t*>(base + (size_t)r * p.src_step + (size_t)c * 4);
      }
    }
  };
  if (interior) load_tile(g);
  for (int f = g; f < p.n_frames; f += groups) {
    const uint8_t* src = p.src + (size_t)f * p.src_frame_stride;
    uint8_t* dst = p.dst + (size_t)f * p.dst_frame_stride;
    if (interior) {
#pragma unroll
      for (int kk = 0; kk < kPre; kk++) {
        const int k = tid + kk * kBlock16, r = k / kLdsDwords, c = k - r * kLdsDwords;
        if constexpr (L::kPacked) {
          if (k < kLdsRows * kLdsDwords) {
            int lo, sh;
            L::locate(tx0, c, lo, sh);
            lds[r * kLdsStride + c] = L::decode(pre[kk], pre_hi[kk], sh, tx0 - 2 + 2 * c);
          }
        } else {
          if (k < kLdsRows * kLdsDwords) lds[r * kLdsStride + c] = pre[kk];
        }
      }
    } else {
      for (int k = tid; k < kLdsRows * kLdsDwords * 2; k += kBlock16) {
        const int r = k / (kLdsDwords * 2), c = k - r * (kLdsDwords * 2);
        const int y = reflect101(ty0 - 2 + r, p.rows), x = reflect101(tx0 - 2 + c, p.cols);
        lds16[r * (2 * kLdsStride) + c] = (uint16_t)L::sample(src + (size_t)y * p.src_step, x);
      }
    }
    __syncthreads();
    if (interior && f + groups < p.n_frames) load_tile(f + groups);
    if (active) {
      // val[i][q][c]: output row i, pixel q, channel c (0 B, 1 G, 2 R), 16-bit range (MHT: not yet clamped)
      int val[2][4][3];
      if (!MHT && !interior) {
        // block-uniform.  Bilinear's border rule -- the formula at the position clamped to [1, n - 2], whose Bayer phase is
        // another -- on every pixel of a tile that touches the frame's edge: identity away from the outermost rows and columns
#pragma unroll
        for (int i = 0; i < 2; i++) {
          const int yc = min(max(y0 + i, 1), p.rows - 2);
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const int xc = min(max(x0 + q, 1), p.cols - 2);
            bilinear_at(lds16, yc - ty0 + 2, xc - tx0 + 2, (yc - RY) & 1, (xc - RX) & 1, val[i][q][0], val[i][q][1], val[i][q][2]);
          }
        }
      } else {
        // S[r][k]: row y0 - 2 + r, sample x0 - 2 + k
        int S[6][8];
#pragma unroll
        for (int r = 0; r < 6; r++) {
          const uint32_t* row = lds + (2 * ly + r) * kLdsStride + 2 * lx;
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const uint32_t d = row[k];
            S[r][2 * k] = (int)(d & 0xFFFFu);
            S[r][2 * k + 1] = (int)(d >> 16);
          }
        }
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const int dy = (i + RY) & 1, dx = (q + RX) & 1;
            const int c = S[i + 2][q + 2];
            const int h1 = S[i + 2][q + 1] + S[i + 2][q + 3], v1 = S[i + 1][q + 2] + S[i + 3][q + 2];
            const int d = (S[i + 1][q + 1] + S[i + 1][q + 3]) + (S[i + 3][q + 1] + S[i + 3][q + 3]);
            int r, gr, b;
            if constexpr (MHT) {
              const int h2 = S[i + 2][q] + S[i + 2][q + 4], v2 = S[i][q + 2] + S[i + 4][q + 2];
              if (dy == dx) {  // R (0, 0) or B (1, 1) site: K_G and K_diag
                gr = mht_round16(8 * c + 4 * (h1 + v1) - 2 * (h2 + v2));
                const int o = mht_round16(12 * c + 4 * d - 3 * (h2 + v2));
                r = dy == 0 ? c : o;
                b = dy == 0 ? o : c;
              } else {  // G site: K_row for the colour of the left / right neighbours, K_col for the upper / lower ones
                const int rs = mht_round16(10 * c + 8 * h1 - 2 * h2 + v2 - 2 * d);
                const int cs = mht_round16(10 * c + 8 * v1 + h2 - 2 * v2 - 2 * d);
                gr = c;
                r = dy == 0 ? rs : cs;
                b = dy == 0 ? cs : rs;
              }
            } else {
              if (dy != dx) {
                const int h = (h1 + 1) >> 1, vv = (v1 + 1) >> 1;
                gr = c;
                r = dy == 0 ? h : vv;
                b = dy == 0 ? vv : h;
              } else {
                const int d4 = (d + 2) >> 2;
                gr = (h1 + v1 + 2) >> 2;
                r = dy == 0 ? c : d4;
                b = dy == 0 ? d4 : c;
              }
            }
            val[i][q][0] = b;
            val[i][q][1] = gr;
            val[i][q][2] = r;
          }
        }
      }
      uint32_t nb[2][4][3];
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
          for (int c = 0; c < 3; c++) nb[i][q][c] = narrow(val[i][q][c]);
#pragma unroll
      for (int i = 0; i < 2; i++) {
        // destination order: mirrored for the 180-degree flip
        auto o = [&](int k) -> uint32_t { const int q = k / 3, c = k - q * 3; return nb[i][kFlip180 ? 3 - q : q][c]; };
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
            ob[0] = (uint8_t)nb[i][q][0];
            ob[1] = (uint8_t)nb[i][q][1];
            ob[2] = (uint8_t)nb[i][q][2];
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
      for (int k = tid; k < kTileW * (kTileH / 4); k += kBlock16) {
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

template <class L, bool MHT, int RY, int RX>
void launch_angle(const Raw16Params& p, dim3 grid, hipStream_t stream) {
  if (t_launch_log != nullptr) {  // the layout class as the demangler prints it
    char layout[24];
    if (L::kPacked) std::snprintf(layout, sizeof(layout), "StagePacked<%d>", L::kLayout);
    else std::snprintf(layout, sizeof(layout), "StageU16");
    RIP_LOG_LAUNCH(grid, kBlock16, p.n_frames, "raw16_tile_kernel<%s, %s, %d, %d, %d>", layout, launch_log_bool(MHT), RY, RX, p.flip_angle);
  }
  switch (p.flip_angle) {
    case 90: hipLaunchKernelGGL((raw16_tile_kernel<L, MHT, RY, RX, 90>), grid, dim3(kBlock16), 0, stream, p); break;
    case 180: hipLaunchKernelGGL((raw16_tile_kernel<L, MHT, RY, RX, 180>), grid, dim3(kBlock16), 0, stream, p); break;
    case 270: hipLaunchKernelGGL((raw16_tile_kernel<L, MHT, RY, RX, 270>), grid, dim3(kBlock16), 0, stream, p); break;
    default: hipLaunchKernelGGL((raw16_tile_kernel<L, MHT, RY, RX, 0>), grid, dim3(kBlock16), 0, stream, p); break;
  }
}

template <class L, bool MHT>
void launch_phase(const Raw16Params& p, dim3 grid, hipStream_t stream) {
  const int phase = p.bayer_ry * 2 + p.bayer_rx;
  if (phase == 0) launch_angle<L, MHT, 0, 0>(p, grid, stream);
  else if (phase == 1) launch_angle<L, MHT, 0, 1>(p, grid, stream);
  else if (phase == 2) launch_angle<L, MHT, 1, 0>(p, grid, stream);
  else launch_angle<L, MHT, 1, 1>(p, grid, stream);
}

bool aligned4p(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 3u) == 0; }

// the launch of either file: the narrowing's constants, the alignment flags, the frame groups and the grid
template <class L>
void launch_tiles(const Raw16Params& p_in, hipStream_t stream) {
  if (p_in.n_frames <= 0) return;
  Raw16Params p = p_in;
  const int a = p.flip_angle == 90 || p.flip_angle == 180 || p.flip_angle == 270 ? p.flip_angle : 0;
  p.flip_angle = a;
  p.range = p.white - p.black;
  raw16_narrow_constants(p.black, p.white, &p.mul, &p.shift);
  p.src_aligned4 = aligned4p(p.src) && p.src_step % 4 == 0 && p.src_frame_stride % 4 == 0;
  // 4-aligned dword stores: a quarter turn by 90 starts its 32-px segments at rows - 32 - ty0
  p.dst_aligned4 = aligned4p(p.dst) && p.dst_step % 4 == 0 && p.dst_frame_stride % 4 == 0 && (a != 180 || p.cols % 4 == 0) &&
                   (a != 90 || p.rows % 4 == 0);
  const long long tiles = (long long)((p.cols + kTileW - 1) / kTileW) * ((p.rows + kTileH - 1) / kTileH);
  // kFramesPerBlock frames per workgroup visit; fewer groups (more frames per visit) if the 1-D grid would overflow
  const long long max_groups = std::max(1LL, 0x7fffff00LL / tiles);
  p.frame_groups = (int)std::min<long long>((p.n_frames + kFramesPerBlock - 1) / kFramesPerBlock, max_groups);
  const long long grid = ((tiles * p.frame_groups) + kXcds - 1) / kXcds * kXcds;
  if (p.mht) launch_phase<L, true>(p, dim3((unsigned)grid), stream);
  else launch_phase<L, false>(p, dim3((unsigned)grid), stream);
}

}  // namespace
}  // namespace rip
