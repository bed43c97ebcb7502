// rip_unpack.hpp -- packed 10- / 12-bit Bayer rows (rip.h "Packed Bayer frames"): the layouts, their geometry rule and the
// extract functions, shared by the kernels' byte path (rip_raw16_dev.hpp), the host layer (rip_plan.cpp: row bytes, the checks)
// and rip_debug_unpack, which pins this arithmetic on the CPU.
//
// Sample x of a row of bytes b[0..]:
//   10p       PFNC lsb-first bit stream: bits [10 x, 10 x + 10) of the row read as a little-endian bit string.  10 x & 7 is 0, 2,
//             4 or 6, so the sample lies in the two bytes b[k], b[k + 1], k = 10 x >> 3
//   12p       the same with 12 bits: k = 12 x >> 3, even x: b[k] | (b[k + 1] & 15) << 8, odd x: b[k] >> 4 | b[k + 1] << 4
//   10_csi2   MIPI CSI-2 RAW10: groups of 4 samples in 5 bytes, g = x >> 2, j = x & 3: b[5 g + j] << 2 | (b[5 g + 4] >> 2 j) & 3
//   12_csi2   MIPI CSI-2 RAW12: groups of 2 samples in 3 bytes, g = x >> 1: even x: b[3 g] << 4 | b[3 g + 2] & 15,
//             odd x: b[3 g + 1] << 4 | b[3 g + 2] >> 4
// No function here reads a byte the sample does not lie in.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RIP_HD __host__ __device__ __forceinline__
#else
#define RIP_HD inline
#endif

namespace rip {

enum PackedLayout { PACKED_NONE = 0, PACKED_10P = 1, PACKED_12P = 2, PACKED_10_CSI2 = 3, PACKED_12_CSI2 = 4 };

RIP_HD int packed_bits(int layout) { return layout == PACKED_10P || layout == PACKED_10_CSI2 ? 10 : 12; }
// cols must be a multiple of this (whole CSI-2 groups); the p layouts take any width
RIP_HD int packed_cols_multiple(int layout) { return layout == PACKED_10_CSI2 ? 4 : layout == PACKED_12_CSI2 ? 2 : 1; }
RIP_HD size_t packed_row_bytes(int layout, int cols) { return ((size_t)cols * (size_t)packed_bits(layout) + 7) >> 3; }

RIP_HD uint32_t unpack_10p(const uint8_t* b, int x) {
  const int bit = 10 * x, k = bit >> 3;
  const uint32_t w = (uint32_t)b[k] | (uint32_t)b[k + 1] << 8;
  return (w >> (bit & 7)) & 0x3FFu;
}
RIP_HD uint32_t unpack_12p(const uint8_t* b, int x) {
  const int k = (12 * x) >> 3;
  const uint32_t lo = b[k], hi = b[k + 1];
  return (x & 1) ? (lo >> 4 | hi << 4) : (lo | (hi & 15u) << 8);
}
RIP_HD uint32_t unpack_10_csi2(const uint8_t* b, int x) {
  const int g = x >> 2, j = x & 3;
  const uint32_t hi = b[5 * g + j], lo = b[5 * g + 4];
  return hi << 2 | ((lo >> (2 * j)) & 3u);
}
RIP_HD uint32_t unpack_12_csi2(const uint8_t* b, int x) {
  const int g = x >> 1;
  const uint32_t lo = b[3 * g + 2];
  return (x & 1) ? ((uint32_t)b[3 * g + 1] << 4 | lo >> 4) : ((uint32_t)b[3 * g] << 4 | (lo & 15u));
}

template <int LAYOUT>
RIP_HD uint32_t unpack_sample(const uint8_t* b, int x) {
  if (LAYOUT == PACKED_10P) return unpack_10p(b, x);
  if (LAYOUT == PACKED_12P) return unpack_12p(b, x);
  if (LAYOUT == PACKED_10_CSI2) return unpack_10_csi2(b, x);
  return unpack_12_csi2(b, x);
}

}  // namespace rip
