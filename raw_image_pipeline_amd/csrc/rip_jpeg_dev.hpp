// rip_jpeg_dev.hpp -- the device code of rip_jpeg.hip and the checks its launch functions make (PARITY.md "Output formats: JPEG").
// Included by rip_jpeg.hip alone.  No kernel uses LDS, a barrier or a cross-lane operation: every lane works on its own item -- a
// block, a restart interval, a frame -- so the same code runs lane by lane on the host (tests/cpp/jpeg_kernel_host.cpp).
//
// The entropy coder is one function template, jpeg_code_interval<Write>: the sizing pass and the writing pass run the same
// statements over the same coefficients, so the bytes the second one stores are the bytes the first one counted.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rip_jpeg.hpp"

namespace rip {
namespace {

typedef uint32_t jpeg_u32x4 __attribute__((ext_vector_type(4)));

// position in zigzag order of the coefficient at natural (row-major) index n.  constexpr: in the transform's unrolled loop every
// index into the packed words is a compile-time constant, so the words stay in registers (0 bytes of scratch in both instantiations)
constexpr uint8_t kJpegZigzagOf[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                              10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// round(c * 2^13) of the twelve constants of the transform
constexpr int kF0298 = 2446, kF0390 = 3196, kF0541 = 4433, kF0765 = 6270, kF0899 = 7373, kF1175 = 9633;
constexpr int kF1501 = 12299, kF1847 = 15137, kF1961 = 16069, kF2053 = 16819, kF2562 = 20995, kF3072 = 25172;

__device__ __forceinline__ int jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One pass of the transform over d[0], d[stride], ..: the first (rows) keeps two more bits, the second (columns) removes them
template <bool First>
__device__ __forceinline__ void jpeg_dct_pass(int* d, int stride) {
  constexpr int n = First ? 11 : 15;
  const int t0 = d[0] + d[7 * stride], t7 = d[0] - d[7 * stride];
  const int t1 = d[stride] + d[6 * stride], t6 = d[stride] - d[6 * stride];
  const int t2 = d[2 * stride] + d[5 * stride], t5 = d[2 * stride] - d[5 * stride];
  const int t3 = d[3 * stride] + d[4 * stride], t4 = d[3 * stride] - d[4 * stride];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if constexpr (First) {
    d[0] = (t10 + t11) * 4;
    d[4 * stride] = (t10 - t11) * 4;
  } else {
    d[0] = jpeg_descale(t10 + t11, 2);
    d[4 * stride] = jpeg_descale(t10 - t11, 2);
  }
  const int e1 = (t12 + t13) * kF0541;
  d[2 * stride] = jpeg_descale(e1 + t13 * kF0765, n);
  d[6 * stride] = jpeg_descale(e1 - t12 * kF1847, n);
  const int z5 = (t4 + t6 + t5 + t7) * kF1175;
  const int z1 = -(t4 + t7) * kF0899, z2 = -(t5 + t6) * kF2562;
  const int z3 = -(t4 + t6) * kF1961 + z5, z4 = -(t5 + t7) * kF0390 + z5;
  d[7 * stride] = jpeg_descale(t4 * kF0298 + z1 + z3, n);
  d[5 * stride] = jpeg_descale(t5 * kF2053 + z2 + z4, n);
  d[3 * stride] = jpeg_descale(t6 * kF3072 + z2 + z3, n);
  d[stride] = jpeg_descale(t7 * kF1501 + z1 + z4, n);
}

// packed[z >> 1] |= bits << (16 * (z & 1)) for z = kJpegZigzagOf[n]; n is a constant after unrolling, and so is z
__device__ __forceinline__ void jpeg_zigzag_or(uint32_t* packed, int n, uint32_t bits) {
  const int z = kJpegZigzagOf[n];
  packed[z >> 1] |= bits << (16 * (z & 1));
}

// ---- jpeg_transform_kernel ------------------------------------------------------------------------------------------------------
// grid (ceil(blocks / 64), 1, frames).  Lane b of a frame owns block b in scan order: MCU b / 6 (or b), and inside a colour MCU the
// four luminance blocks row by row, then Cb, then Cr.  Samples beyond the picture repeat its last column and row.
template <bool Colour>
__device__ __forceinline__ void jpeg_transform(const JpegParams& p) {
  constexpr int per_mcu = Colour ? 6 : 1;
  const int mcux = jpeg_mcus_x(p.cols, p.channels), mcuy = jpeg_mcus_y(p.rows, p.channels);
  const unsigned blocks = (unsigned)mcux * (unsigned)mcuy * per_mcu;
  const unsigned b = blockIdx.x * kJpegBlock + threadIdx.x;
  if (b >= blocks) return;
  const int mcu = (int)(b / per_mcu), k = (int)(b % per_mcu);
  const int my = mcu / mcux, mx = mcu % mcux;
  const uint8_t* frame = p.src + (size_t)blockIdx.z * p.src_frame_stride;
  int v[64];
  if constexpr (!Colour) {
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const uint8_t* row = frame + (size_t)min(my * 8 + r, p.rows - 1) * p.src_step;
#pragma unroll
      for (int c = 0; c < 8; c++) v[r * 8 + c] = (int)row[min(mx * 8 + c, p.cols - 1)] - 128;
    }
  } else if (k < 4) {
    const int y0 = my * 16 + (k >> 1) * 8, x0 = mx * 16 + (k & 1) * 8;
    const int ybias = (p.m.yoff << 15) + 16384;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const uint8_t* row = frame + (size_t)min(y0 + r, p.rows - 1) * p.src_step;
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const uint8_t* px = row + (size_t)min(x0 + c, p.cols - 1) * 3;
        v[r * 8 + c] = ((p.m.y[0] * (int)px[0] + p.m.y[1] * (int)px[1] + p.m.y[2] * (int)px[2] + ybias) >> 15) - 128;
      }
    }
  } else {
    const int* w = k == 4 ? p.m.cb : p.m.cr;
    const int w0 = w[0], w1 = w[1], w2 = w[2];
    const int cbias = (128 << 17) + 65536;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const uint8_t* row0 = frame + (size_t)min(my * 16 + 2 * r, p.rows - 1) * p.src_step;
      const uint8_t* row1 = frame + (size_t)min(my * 16 + 2 * r + 1, p.rows - 1) * p.src_step;
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const size_t xa = (size_t)min(mx * 16 + 2 * c, p.cols - 1) * 3, xb = (size_t)min(mx * 16 + 2 * c + 1, p.cols - 1) * 3;
        const int sb = (int)row0[xa] + (int)row0[xb] + (int)row1[xa] + (int)row1[xb];
        const int sg = (int)row0[xa + 1] + (int)row0[xb + 1] + (int)row1[xa + 1] + (int)row1[xb + 1];
        const int sr = (int)row0[xa + 2] + (int)row0[xb + 2] + (int)row1[xa + 2] + (int)row1[xb + 2];
        v[r * 8 + c] = min(255, (w0 * sb + w1 * sg + w2 * sr + cbias) >> 17) - 128;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 8; r++) jpeg_dct_pass<true>(v + r * 8, 1);
#pragma unroll
  for (int c = 0; c < 8; c++) jpeg_dct_pass<false>(v + c, 8);
  // round to nearest, ties away from zero, of v / (8 Q) without a division; zigzag
  const int t = Colour && k >= 4 ? 1 : 0;
  const uint32_t* recip = p.tables->recip[t];
  const uint32_t* half = p.tables->half[t];
  uint32_t packed[32];
#pragma unroll
  for (int i = 0; i < 32; i++) packed[i] = 0u;
#pragma unroll
  for (int n = 0; n < 64; n++) {
    const int c = v[n];
    const uint32_t a = (uint32_t)(c < 0 ? -c : c) + half[n];
    const int q = min((int)(((uint64_t)a * recip[n]) >> 32), kJpegMaxCoefficient);
    const uint32_t bits = (uint32_t)(c < 0 ? -q : q) & 0xFFFFu;
    jpeg_zigzag_or(packed, n, bits);
  }
  // 128 bytes per block, 16-byte aligned: the scratch is hipMalloc'ed and a block starts a multiple of 128 bytes into it
  jpeg_u32x4* out = reinterpret_cast<jpeg_u32x4*>(p.coef + ((size_t)blockIdx.z * blocks + b) * 64);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = jpeg_u32x4{packed[4 * i], packed[4 * i + 1], packed[4 * i + 2], packed[4 * i + 3]};
}

// ---- the entropy coder ----------------------------------------------------------------------------------------------------------
// Bits enter at the low end of `acc`; whole bytes leave from its high end, a 0x00 behind every 0xFF.  Write = false counts only.
template <bool Write>
struct JpegSink {
  uint8_t* out;
  uint32_t acc = 0, n = 0, bytes = 0;
  __device__ __forceinline__ explicit JpegSink(uint8_t* o) : out(o) {}
  __device__ __forceinline__ void byte(uint32_t b) {
    if constexpr (Write) out[bytes] = (uint8_t)b;
    bytes++;
  }
  // len <= 16 bits of `code`; at most 7 bits wait in acc, so 23 fit
  __device__ __forceinline__ void put(uint32_t code, uint32_t len) {
    acc = (acc << len) | code;
    n += len;
    while (n >= 8) {
      const uint32_t b = (acc >> (n - 8)) & 255u;
      byte(b);
      if (b == 255u) byte(0u);
      n -= 8;
    }
    acc &= (1u << n) - 1u;
  }
  __device__ __forceinline__ void pad() {
    if (n) put((1u << (8 - n)) - 1u, 8 - n);
  }
};

__device__ __forceinline__ uint32_t jpeg_category(int a) { return a ? 32u - (uint32_t)__builtin_clz((unsigned)a) : 0u; }

// the value bits of v in `size` bits: v, or v - 1 for a negative one
template <bool Write>
__device__ __forceinline__ void jpeg_put_value(JpegSink<Write>& s, uint32_t entry, int v, uint32_t size) {
  s.put(entry & 0xFFFFu, entry >> 16);
  if (size) s.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u), size);
}

// one block: 64 zigzag-ordered coefficients, 16-byte aligned; pred: the component's DC of the block before
template <bool Write>
__device__ __forceinline__ void jpeg_code_block(JpegSink<Write>& s, const int16_t* coef, int& pred, const uint32_t* dc, const uint32_t* ac) {
  int run = 0;
  // the block's eight 16-byte loads are issued together: a lane's blocks lie far from its neighbours', so each load is a trip of its
  // own and one at a time would leave the lane waiting eight times per block
  jpeg_u32x4 w[8];
#pragma unroll
  for (int g = 0; g < 8; g++) w[g] = reinterpret_cast<const jpeg_u32x4*>(coef)[g];
#pragma unroll
  for (int g = 0; g < 8; g++) {
    const uint32_t words[4] = {w[g].x, w[g].y, w[g].z, w[g].w};
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int v = (int)(int16_t)(words[i >> 1] >> (16 * (i & 1)));
      if (g == 0 && i == 0) {
        const int diff = v - pred;
        pred = v;
        const uint32_t size = jpeg_category(diff < 0 ? -diff : diff);
        jpeg_put_value(s, dc[size], diff, size);
        continue;
      }
      if (v == 0) {
        run++;
        continue;
      }
      while (run > 15) {
        s.put(ac[0xF0] & 0xFFFFu, ac[0xF0] >> 16);
        run -= 16;
      }
      const uint32_t size = jpeg_category(v < 0 ? -v : v);
      jpeg_put_value(s, ac[((uint32_t)run << 4) | size], v, size);
      run = 0;
    }
  }
  if (run) s.put(ac[0] & 0xFFFFu, ac[0] >> 16);  // EOB
}

// Restart interval `iv` of frame `f`: its MCU rows, padded with 1-bits to a byte, RSTm behind every interval but the last.
// Returns the bytes; Write: stored from `out` on.
template <bool Write>
__device__ __forceinline__ uint32_t jpeg_code_interval(const JpegParams& p, int f, int iv, uint8_t* out) {
  const int per_mcu = jpeg_blocks_per_mcu(p.channels);
  const int mcux = jpeg_mcus_x(p.cols, p.channels), mcuy = jpeg_mcus_y(p.rows, p.channels);
  const int row0 = iv * p.restart_rows, row1 = min(row0 + p.restart_rows, mcuy);
  const size_t blocks = (size_t)mcux * mcuy * per_mcu;
  const int16_t* coef = p.coef + ((size_t)f * blocks + (size_t)row0 * mcux * per_mcu) * 64;
  JpegSink<Write> s(out);
  int pred[3] = {0, 0, 0};
  const JpegTables* t = p.tables;
#pragma unroll 1
  for (int mcu = 0; mcu < (row1 - row0) * mcux; mcu++) {
    if (per_mcu == 1) {
      jpeg_code_block(s, coef, pred[0], t->dc[0], t->ac[0]);
      coef += 64;
    } else {
#pragma unroll 1
      for (int k = 0; k < 4; k++, coef += 64) jpeg_code_block(s, coef, pred[0], t->dc[0], t->ac[0]);
      jpeg_code_block(s, coef, pred[1], t->dc[1], t->ac[1]);
      jpeg_code_block(s, coef + 64, pred[2], t->dc[1], t->ac[1]);
      coef += 128;
    }
  }
  s.pad();
  if (row1 < mcuy) {
    s.byte(255u);
    s.byte(0xD0u + ((uint32_t)iv & 7u));
  }
  return s.bytes;
}

// ---- jpeg_size_kernel: grid (ceil(intervals / 64), 1, frames) -------------------------------------------------------------------
__device__ __forceinline__ void jpeg_size(const JpegParams& p) {
  const int intervals = jpeg_intervals(p.rows, p.channels, p.restart_rows);
  const int iv = (int)(blockIdx.x * kJpegBlock + threadIdx.x);
  if (iv >= intervals) return;
  p.intervals[(size_t)blockIdx.z * intervals + iv] = jpeg_code_interval<false>(p, (int)blockIdx.z, iv, nullptr);
}

// ---- jpeg_scan_kernel: grid (ceil(frames / 64), 1, 1) ---------------------------------------------------------------------------
// Turns a frame's byte counts into offsets behind the header, in place, and decides: header + scan + EOI fits the slot, or size 0.
__device__ __forceinline__ void jpeg_scan(const JpegParams& p) {
  const int intervals = jpeg_intervals(p.rows, p.channels, p.restart_rows);
  const int f = (int)(blockIdx.x * kJpegBlock + threadIdx.x);
  if (f >= p.n_frames) return;
  uint32_t* iv = p.intervals + (size_t)f * intervals;
  uint64_t at = 0;
#pragma unroll 1
  for (int i = 0; i < intervals; i++) {
    const uint32_t n = iv[i];
    iv[i] = (uint32_t)(at < 0xFFFFFFFFull ? at : 0xFFFFFFFFull);
    at += n;
  }
  const uint64_t total = (uint64_t)jpeg_header_bytes(p.channels) + at + 2;
  p.sizes[f] = total <= (uint64_t)p.dst_step ? (uint32_t)total : 0u;
}

// ---- jpeg_write_kernel: grid (ceil(intervals / 64) + 1, 1, frames) --------------------------------------------------------------
// The last workgroup of a frame copies the header and writes EOI; the lanes of the others write one interval each.
__device__ __forceinline__ void jpeg_write(const JpegParams& p) {
  const int intervals = jpeg_intervals(p.rows, p.channels, p.restart_rows);
  const int f = (int)blockIdx.z;
  const uint32_t size = p.sizes[f];
  if (size == 0u) return;  // the stream does not fit: the slot keeps its contents
  uint8_t* slot = p.dst + (size_t)f * p.dst_frame_stride;
  const int header = jpeg_header_bytes(p.channels);
  if (blockIdx.x + 1 == gridDim.x) {
    for (int i = (int)threadIdx.x; i < header; i += kJpegBlock) slot[i] = p.header[i];
    if (threadIdx.x == 0) {
      slot[size - 2] = 0xFF;
      slot[size - 1] = 0xD9;
    }
    return;
  }
  const int iv = (int)(blockIdx.x * kJpegBlock + threadIdx.x);
  if (iv >= intervals) return;
  (void)jpeg_code_interval<true>(p, f, iv, slot + header + p.intervals[(size_t)f * intervals + iv]);
}

// ---- the launch checks ----------------------------------------------------------------------------------------------------------
inline bool jpeg_ok(const JpegParams& p) {
  if (!p.src || !p.dst || !p.tables || !p.header || !p.coef || !p.intervals || !p.sizes) return false;
  if (p.rows < 1 || p.cols < 1 || p.rows > 65535 || p.cols > 65535 || (p.channels != 1 && p.channels != 3)) return false;
  if (p.n_frames < 1 || p.n_frames > 65535 || p.restart_rows < 1 || p.restart_rows > 64) return false;
  if ((long long)p.restart_rows * jpeg_mcus_x(p.cols, p.channels) > 65535) return false;
  if (p.src_step < (size_t)p.cols * p.channels) return false;
  if (p.dst_step < (size_t)jpeg_header_bytes(p.channels) + 2 || p.dst_step > 0xFFFFFFFFull || p.dst_frame_stride < p.dst_step) return false;
  if (reinterpret_cast<uintptr_t>(p.coef) & 15) return false;
  return true;
}

}  // namespace
}  // namespace rip
