// rip_jpeg.hpp -- the JPEG output format (rip_set_output_format "jpeg", rip_set_output_jpeg; PARITY.md "Output formats: JPEG"): the
// delivered 8-bit picture as a baseline JFIF stream, YCbCr 4:2:0 from B, G, R or one component from a one-channel picture, encoded
// on the device.  Four kernels in a library of their own, librip_jpeg_hip.so (rip_jpeg.hip; device code rip_jpeg_dev.hpp):
//   jpeg_transform_kernel<Colour>  picture -> quantised coefficients, one 8 x 8 block per lane: colour conversion, edge repetition and
//                                  the 2 x 2 chroma sums in the load, the integer forward DCT, the reciprocal quantiser, zigzag
//   jpeg_size_kernel               coefficients -> the stuffed byte count of every restart interval, one interval per lane
//   jpeg_scan_kernel               byte counts -> offsets, the stream length of every frame and the overflow decision, one frame per lane
//   jpeg_write_kernel              coefficients -> the bytes of every interval at their final position, one interval per lane; one
//                                  further workgroup per frame copies the header and writes EOI.  A frame of length 0 is not touched.
// This header is the library's whole interface: plain data, the host's table and header builders, and one launch function each.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rip_launch_info.hpp"
#include "rip_yuv.hpp"

namespace rip {

constexpr int kJpegBlock = 64;           // lanes of a workgroup of every kernel
constexpr int kJpegHeaderGrey = 330;     // bytes from SOI up to and including SOS
constexpr int kJpegHeaderColour = 613;
constexpr int kJpegMaxCoefficient = 1023;  // quantised values are clamped to +-1023: AC category <= 10, DC difference category <= 11

// What the kernels read besides the picture, built by jpeg_build_tables and kept on the device
struct JpegTables {
  uint32_t recip[2][64];  // luminance / chrominance, natural (row-major) order: ceil(2^32 / (8 Q))
  uint32_t half[2][64];   // 4 Q
  uint32_t dc[2][12];     // by category: code | length << 16
  uint32_t ac[2][256];    // by run << 4 | size: code | length << 16; 0 where Annex K has no code
};

struct JpegParams {
  // the delivered picture: interleaved B, G, R (channels 3) or one channel of uint8, rows x cols, any alignment
  const uint8_t* src;
  size_t src_step, src_frame_stride;
  // the caller's slots: frame f's stream starts at dst + f * dst_frame_stride, any alignment; dst_step is the capacity of a slot
  uint8_t* dst;
  size_t dst_step, dst_frame_stride;
  int rows, cols, channels, n_frames;
  int restart_rows;  // MCU rows per restart interval
  YuvMatrix m;       // bt601_full; read for three channels
  const JpegTables* tables;
  const uint8_t* header;  // kJpegHeaderGrey / kJpegHeaderColour bytes (jpeg_build_header)
  // scratch: jpeg_coef_bytes / jpeg_interval_bytes of it; sizes: n_frames words that outlive the call
  int16_t* coef;
  uint32_t* intervals;
  uint32_t* sizes;
};

// ---- geometry -----------------------------------------------------------------------------------------------------------------
constexpr int jpeg_mcu(int channels) { return channels == 3 ? 16 : 8; }
constexpr int jpeg_blocks_per_mcu(int channels) { return channels == 3 ? 6 : 1; }
constexpr int jpeg_mcus_x(int cols, int channels) { return (cols + jpeg_mcu(channels) - 1) / jpeg_mcu(channels); }
constexpr int jpeg_mcus_y(int rows, int channels) { return (rows + jpeg_mcu(channels) - 1) / jpeg_mcu(channels); }
constexpr int jpeg_intervals(int rows, int channels, int restart_rows) { return (jpeg_mcus_y(rows, channels) + restart_rows - 1) / restart_rows; }
constexpr int jpeg_header_bytes(int channels) { return channels == 3 ? kJpegHeaderColour : kJpegHeaderGrey; }
inline size_t jpeg_blocks(int rows, int cols, int channels) { return (size_t)jpeg_mcus_x(cols, channels) * jpeg_mcus_y(rows, channels) * jpeg_blocks_per_mcu(channels); }
// the default slot: header + one byte per coded sample of the extended picture + 2 per restart interval + 2
inline size_t jpeg_default_slot(int rows, int cols, int channels, int restart_rows) {
  return (size_t)jpeg_header_bytes(channels) + jpeg_blocks(rows, cols, channels) * 64 + 2 * (size_t)jpeg_intervals(rows, channels, restart_rows) + 2;
}
inline size_t jpeg_coef_bytes(int rows, int cols, int channels, int n_frames) { return jpeg_blocks(rows, cols, channels) * 128 * (size_t)n_frames; }
inline size_t jpeg_interval_bytes(int rows, int channels, int restart_rows, int n_frames) { return (size_t)jpeg_intervals(rows, channels, restart_rows) * 4 * (size_t)n_frames; }

// ---- the tables of Annex K ----------------------------------------------------------------------------------------------------
namespace jpeg_annex_k {
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24, 40, 51,  61,  12, 12, 14, 19, 26, 58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
}  // namespace jpeg_annex_k

// the divisor Q of base value `base` under `quality` (1..100), the IJG rule
inline int jpeg_quant_value(int base, int quality) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int q = (base * s + 50) / 100;
  return q < 1 ? 1 : (q > 255 ? 255 : q);
}

// Fills the tables for a quality; q_out (optional): the 2 x 64 divisors in natural order
inline void jpeg_build_tables(int quality, JpegTables& t, uint8_t* q_out = nullptr) {
  using namespace jpeg_annex_k;
  for (int c = 0; c < 2; c++)
    for (int n = 0; n < 64; n++) {
      const int q = jpeg_quant_value(c ? kBaseChroma[n] : kBaseLuma[n], quality);
      const uint64_t d = 8u * (uint64_t)q;
      t.recip[c][n] = (uint32_t)(((1ull << 32) + d - 1) / d);
      t.half[c][n] = 4u * (uint32_t)q;
      if (q_out) q_out[c * 64 + n] = (uint8_t)q;
    }
  for (int c = 0; c < 2; c++) {
    for (int cls = 0; cls < 2; cls++) {
      const uint8_t* bits = cls ? kAcBits[c] : kDcBits[c];
      uint32_t* out = cls ? t.ac[c] : t.dc[c];
      for (int i = 0; i < (cls ? 256 : 12); i++) out[i] = 0;
      uint32_t code = 0;
      int k = 0;
      for (int len = 1; len <= 16; len++) {  // Annex C: codes of a length are consecutive, the first of the next length is doubled
        for (int i = 0; i < bits[len - 1]; i++, k++, code++) out[cls ? kAcVals[c][k] : k] = code | ((uint32_t)len << 16);
        code <<= 1;
      }
    }
  }
}

// Writes the header -- SOI, APP0 (JFIF 1.01, density 1:1), DQT, SOF0, DHT, DRI, SOS -- of a rows x cols picture into `out`
// (jpeg_header_bytes(channels) bytes); q: jpeg_build_tables' divisors.  Returns the bytes written.
inline int jpeg_build_header(int rows, int cols, int channels, int restart_rows, const uint8_t* q, uint8_t* out) {
  using namespace jpeg_annex_k;
  const int nt = channels == 3 ? 2 : 1;
  uint8_t* o = out;
  auto put = [&](int v) { *o++ = (uint8_t)v; };
  auto put16 = [&](int v) { put(v >> 8), put(v & 255); };
  put16(0xFFD8);
  put16(0xFFE0), put16(16);
  for (int v : {0x4A, 0x46, 0x49, 0x46, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0}) put(v);  // "JFIF", 1.01, no units, 1 : 1, no thumbnail
  put16(0xFFDB), put16(2 + 65 * nt);
  for (int c = 0; c < nt; c++) {
    put(c);
    for (int k = 0; k < 64; k++) put(q[c * 64 + kZigzag[k]]);
  }
  put16(0xFFC0), put16(8 + 3 * channels), put(8), put16(rows), put16(cols), put(channels);
  for (int c = 0; c < channels; c++) put(c + 1), put(c == 0 && channels == 3 ? 0x22 : 0x11), put(c ? 1 : 0);
  put16(0xFFC4), put16(2 + nt * (17 + 12 + 17 + 162));
  for (int c = 0; c < nt; c++) {
    put(c);
    for (int i = 0; i < 16; i++) put(kDcBits[c][i]);
    for (int i = 0; i < 12; i++) put(i);
    put(0x10 | c);
    for (int i = 0; i < 16; i++) put(kAcBits[c][i]);
    for (int i = 0; i < 162; i++) put(kAcVals[c][i]);
  }
  put16(0xFFDD), put16(4), put16(restart_rows * jpeg_mcus_x(cols, channels));
  put16(0xFFDA), put16(6 + 2 * channels), put(channels);
  for (int c = 0; c < channels; c++) put(c + 1), put(c ? 0x11 : 0x00);
  put(0), put(63), put(0);
  return (int)(o - out);
}

// Each enqueues one kernel for n_frames frames on `stream`, in this order.  false -- nothing launched -- for a null pointer, an empty
// picture, a channel count other than 1 or 3, a side beyond 65535, restart_rows outside 1..64, a restart interval beyond 65535
// MCUs, a slot below header + 2 or beyond 32 bits, a frame stride below the slot, or more than 65535 frames.
__attribute__((visibility("default"))) bool launch_jpeg_transform(const JpegParams& p, hipStream_t stream, LaunchInfo* info);
__attribute__((visibility("default"))) bool launch_jpeg_size(const JpegParams& p, hipStream_t stream, LaunchInfo* info);
__attribute__((visibility("default"))) bool launch_jpeg_scan(const JpegParams& p, hipStream_t stream, LaunchInfo* info);
__attribute__((visibility("default"))) bool launch_jpeg_write(const JpegParams& p, hipStream_t stream, LaunchInfo* info);

}  // namespace rip
