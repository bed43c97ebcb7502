// rip_clahe_dev.hpp -- the device code of rip_clahe.hip and the checks its launch functions make (PARITY.md "Local contrast:
// CLAHE").  Included by rip_clahe.hip alone.  Both kernels are phase functions around their barriers: every lane of the workgroup
// reaches every barrier, a lane without work leaves the phase, not the kernel, and whatever crosses a barrier or a lane lives in LDS.
//
// clahe_lut_kernel: one workgroup per (tile, frame), grid (tiles_x, tiles_y, frames); LDS: four histograms of 256 counters.
//   lut_zero     the counters
//   lut_count    the tile's th x tw positions of the extended picture, reflect-101 applied to the coordinate.  A lane takes items
//                of four columns that start at a 4-byte aligned address of the row -- one dword where all four lie inside the tile
//                and the picture, single bytes otherwise; the dwords of kClaheLutAhead items are loaded before any is counted -- and
//                keeps a run (value, count) across its items: one LDS atomic add into its wave's histogram per run, so a flat tile
//                costs one add per lane
//   lut_clip     lane k: the sum of bin k over the four histograms, clipped; the clipped count and its excess go back to LDS
//   lut_spread   every lane sums the 256 excesses (broadcast reads), adds its share: batch, and one more by the closed form
//   lut_store    lanes 0 .. 63: the inclusive sums of four neighbouring bins, scaled and rounded, as one dword of the table
// clahe_apply_kernel: grid (1, bands x strips, frames).  Band b = 0 .. tiles_y holds the rows whose upper table row is b - 1
// (clahe_band_start), so one pair (y1c, y2c) per workgroup; a workgroup owns strip_rows rows of its band at the picture's full width.
//   apply_stage  the two table rows, 2 x tiles_x x 256 bytes, from the table block into LDS, dword by dword
//   apply_blend  items of four columns that start at a 4-byte aligned address of the destination row: the pixels are read -- one
//                dword where the source address is aligned too --, then four LDS byte look-ups and the blend per pixel, then one
//                dword store, or single bytes for an item the row's ends cut
// All float32, every product and sum rounded on its own (the library is built with -ffp-contract=off).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rip_clahe.hpp"

namespace rip {

constexpr int kClaheLutAhead = 4;  // items a lane of clahe_lut_kernel loads before it counts them

// floor(v * inv - 0.5f): the table row (column) above (left of) pixel row (column) v, before the clamp
__device__ __forceinline__ int clahe_cell(int v, float inv) { return (int)floorf((float)v * inv - 0.5f); }

// the first row of band b: the smallest y in 0 .. rows with clahe_cell(y) >= b - 1 (the cell is non-decreasing in y).  Starts at the
// exact boundary ceil((b - 1/2) th) and steps over what float32 rounding moved.
__device__ __forceinline__ int clahe_band_start(int b, int th, float inv_th, int rows) {
  long long nominal = ((2LL * b - 1) * th + 1) >> 1;
  int y = (int)(nominal < 0 ? 0 : nominal > rows ? rows : nominal);
  while (y > 0 && clahe_cell(y - 1, inv_th) >= b - 1) y--;
  while (y < rows && clahe_cell(y, inv_th) < b - 1) y++;
  return y;
}

// items of one row: four columns each, the first one starting up to three columns left of column 0
__device__ __forceinline__ int clahe_items_per_row(int cols) { return ((cols + 3) >> 2) + 1; }

// A lane's walk over rows x items_per_row items, kClaheBlock items apart
struct ClaheWalk {
  int row, k, ipr, dq, dm;
  __device__ __forceinline__ ClaheWalk(int lane, int items_per_row) : row(lane / items_per_row), k(lane % items_per_row), ipr(items_per_row), dq(kClaheBlock / items_per_row), dm(kClaheBlock % items_per_row) {}
  __device__ __forceinline__ void next() {
    row += dq;
    k += dm;
    if (k >= ipr) {
      k -= ipr;
      row++;
    }
  }
};

__device__ __forceinline__ int clahe_reflect(int v, int n) { return v < n ? v : max(2 * n - 2 - v, 0); }

__device__ __forceinline__ uint8_t clahe_byte(float v) { return (uint8_t)min(max((int)rintf(v), 0), 255); }

// ---- clahe_lut_kernel ----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void clahe_lut_zero(const ClaheParams&, uint32_t* hist) {
  const int t = (int)threadIdx.x;
#pragma unroll
  for (int w = 0; w < 4; w++) hist[w * kClaheBins + t] = 0u;
}

struct ClaheRun {
  int value;
  uint32_t count;
};
__device__ __forceinline__ void clahe_run_add(ClaheRun& run, int v, uint32_t* h) {
  if (v == run.value) {
    run.count++;
    return;
  }
  if (run.count) atomicAdd(&h[run.value], run.count);
  run.value = v;
  run.count = 1u;
}

__device__ __forceinline__ void clahe_lut_count(const ClaheParams& p, uint32_t* hist) {
  const int t = (int)threadIdx.x;
  uint32_t* h = hist + (t >> 6) * kClaheBins;
  const int x0 = (int)blockIdx.x * p.tw, y0 = (int)blockIdx.y * p.th;
  const uint8_t* frame = p.src + (size_t)blockIdx.z * p.src_frame_stride;
  ClaheRun run = {0, 0u};
  // kClaheLutAhead items per turn: the dwords of the whole ones are all loaded before the first is counted, so a lane has that many
  // loads in flight -- one workgroup per tile is all the parallelism a single frame has
  for (ClaheWalk w(t, clahe_items_per_row(p.tw)); w.row < p.th;) {
    uint32_t v[kClaheLutAhead];
    bool whole[kClaheLutAhead];
#pragma unroll
    for (int u = 0; u < kClaheLutAhead; u++) {
      whole[u] = false;
      v[u] = 0u;
      if (w.row >= p.th) continue;
      const uint8_t* line = frame + (size_t)clahe_reflect(y0 + w.row, p.rows) * p.src_step;
      const int c0 = 4 * w.k - (int)(reinterpret_cast<uintptr_t>(line + x0) & 3);  // the item's first column, counted from the tile's
      if (c0 >= 0 && c0 + 4 <= p.tw && x0 + c0 + 4 <= p.cols) {
        v[u] = *reinterpret_cast<const uint32_t*>(line + x0 + c0);
        whole[u] = true;
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (c0 + i >= 0 && c0 + i < p.tw) clahe_run_add(run, (int)line[clahe_reflect(x0 + c0 + i, p.cols)], h);
      }
      w.next();
    }
#pragma unroll
    for (int u = 0; u < kClaheLutAhead; u++) {
      if (!whole[u]) continue;
#pragma unroll
      for (int i = 0; i < 4; i++) clahe_run_add(run, (int)((v[u] >> (8 * i)) & 255u), h);
    }
  }
  if (run.count) atomicAdd(&h[run.value], run.count);
}

__device__ __forceinline__ void clahe_lut_clip(const ClaheParams& p, uint32_t* hist) {
  const int t = (int)threadIdx.x;
  uint32_t h = hist[t] + hist[kClaheBins + t] + hist[2 * kClaheBins + t] + hist[3 * kClaheBins + t], excess = 0u;
  if (p.clip > 0 && h > (uint32_t)p.clip) {
    excess = h - (uint32_t)p.clip;
    h = (uint32_t)p.clip;
  }
  hist[t] = h;
  hist[kClaheBins + t] = excess;
}

__device__ __forceinline__ void clahe_lut_spread(const ClaheParams& p, uint32_t* hist) {
  const int t = (int)threadIdx.x;
  uint32_t h = hist[t];
  if (p.clip > 0) {
    uint32_t excess = 0u;
    for (int k = 0; k < kClaheBins; k++) excess += hist[kClaheBins + k];
    const uint32_t batch = excess >> 8, residual = excess & 255u;
    h += batch;
    if (residual > 0u) {
      const uint32_t step = max(256u / residual, 1u);
      if ((uint32_t)t % step == 0u && (uint32_t)t / step < residual) h++;
    }
  }
  hist[2 * kClaheBins + t] = h;
}

__device__ __forceinline__ void clahe_lut_store(const ClaheParams& p, const uint32_t* hist) {
  const int t = (int)threadIdx.x;
  if (t >= kClaheBins / 4) return;
  const uint32_t* fin = hist + 2 * kClaheBins;
  uint32_t s = 0u;
  for (int k = 0; k < 4 * t; k++) s += fin[k];
  uint32_t word = 0u;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    s += fin[4 * t + i];
    word |= (uint32_t)clahe_byte((float)s * p.scale) << (8 * i);
  }
  const size_t tile = ((size_t)blockIdx.z * p.tiles_y + blockIdx.y) * p.tiles_x + blockIdx.x;
  reinterpret_cast<uint32_t*>(p.lut + tile * kClaheBins)[t] = word;
}

// ---- clahe_apply_kernel --------------------------------------------------------------------------------------------------------

// the workgroup's band and its rows [y0, y1) of the picture; empty for the strips a short band leaves over
struct ClaheStrip {
  int band, y0, y1;
};
__device__ __forceinline__ int clahe_strips_per_band(const ClaheParams& p, int strip_rows) { return p.th / strip_rows + 1; }  // a band has at most th + 1 rows
__device__ __forceinline__ ClaheStrip clahe_strip(const ClaheParams& p, int strip_rows) {
  const int per_band = clahe_strips_per_band(p, strip_rows);
  ClaheStrip s;
  s.band = (int)blockIdx.y / per_band;
  const int end = clahe_band_start(s.band + 1, p.th, p.inv_th, p.rows);
  s.y0 = min(clahe_band_start(s.band, p.th, p.inv_th, p.rows) + ((int)blockIdx.y % per_band) * strip_rows, end);
  s.y1 = min(s.y0 + strip_rows, end);
  return s;
}

__device__ __forceinline__ void clahe_apply_stage(const ClaheParams& p, int strip_rows, uint8_t* lds) {
  const ClaheStrip s = clahe_strip(p, strip_rows);
  if (s.y0 >= s.y1) return;
  const int row_words = p.tiles_x * (kClaheBins / 4);
  const int j1 = max(s.band - 1, 0), j2 = min(s.band, p.tiles_y - 1);
  const uint32_t* tables = reinterpret_cast<const uint32_t*>(p.lut + (size_t)blockIdx.z * p.tiles_y * p.tiles_x * kClaheBins);
  uint32_t* out = reinterpret_cast<uint32_t*>(lds);
  for (int d = (int)threadIdx.x; d < 2 * row_words; d += kClaheBlock)
    out[d] = d < row_words ? tables[(size_t)j1 * row_words + d] : tables[(size_t)j2 * row_words + (d - row_words)];
}

__device__ __forceinline__ void clahe_apply_blend(const ClaheParams& p, int strip_rows, const uint8_t* lds) {
  const ClaheStrip s = clahe_strip(p, strip_rows);
  if (s.y0 >= s.y1) return;
  const uint8_t* src_frame = p.src + (size_t)blockIdx.z * p.src_frame_stride;
  uint8_t* dst_frame = p.dst + (size_t)blockIdx.z * p.dst_frame_stride;
  const uint8_t* lower = lds + (size_t)p.tiles_x * kClaheBins;  // the tables of row y2c
  for (ClaheWalk w((int)threadIdx.x, clahe_items_per_row(p.cols)); s.y0 + w.row < s.y1; w.next()) {
    const int y = s.y0 + w.row;
    const float fy = (float)y * p.inv_th - 0.5f;
    const float ya = fy - (float)(s.band - 1), ya1 = 1.0f - ya;
    const uint8_t* in = src_frame + (size_t)y * p.src_step;
    uint8_t* out = dst_frame + (size_t)y * p.dst_step;
    const int c0 = 4 * w.k - (int)(reinterpret_cast<uintptr_t>(out) & 3);
    const bool whole = c0 >= 0 && c0 + 4 <= p.cols;
    // every pixel of the item is read before one is written: in place, the item's bytes are this lane's alone
    uint32_t px = 0u;
    if (whole && (reinterpret_cast<uintptr_t>(in + c0) & 3) == 0) {
      px = *reinterpret_cast<const uint32_t*>(in + c0);
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (c0 + i >= 0 && c0 + i < p.cols) px |= (uint32_t)in[c0 + i] << (8 * i);
    }
    uint32_t res = 0u;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int x = c0 + i, v = (int)((px >> (8 * i)) & 255u);
      const float fx = (float)x * p.inv_tw - 0.5f;
      const int x1 = (int)floorf(fx);
      const float xa = fx - (float)x1, xa1 = 1.0f - xa;
      // the weights come from before the clamp; the outer min / max only keep a column outside the picture inside the LDS block
      const int i1 = min(max(x1, 0), p.tiles_x - 1) * kClaheBins + v, i2 = max(min(x1 + 1, p.tiles_x - 1), 0) * kClaheBins + v;
      const float top = (float)lds[i1] * xa1 + (float)lds[i2] * xa;
      const float bottom = (float)lower[i1] * xa1 + (float)lower[i2] * xa;
      res |= (uint32_t)clahe_byte(top * ya1 + bottom * ya) << (8 * i);
    }
    if (whole) {
      *reinterpret_cast<uint32_t*>(out + c0) = res;
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (c0 + i >= 0 && c0 + i < p.cols) out[c0 + i] = (uint8_t)((res >> (8 * i)) & 255u);
    }
  }
}

// ---- the host side: what the launch functions check ----------------------------------------------------------------------------

inline bool clahe_ok(const ClaheParams& p) {
  if (!p.src || !p.dst || !p.lut || (reinterpret_cast<uintptr_t>(p.lut) & 3)) return false;
  if (p.tiles_x < 1 || p.tiles_x > kClaheMaxTiles || p.tiles_y < 1 || p.tiles_y > kClaheMaxTiles) return false;
  if (p.cols < 2 * p.tiles_x || p.rows < 2 * p.tiles_y || p.n_frames < 1 || p.n_frames > 65535) return false;
  if (p.src_step < (size_t)p.cols || p.dst_step < (size_t)p.cols) return false;
  if ((unsigned long long)(p.cols + p.tiles_x) * (unsigned long long)(p.rows + p.tiles_y) >= (1ull << 31)) return false;  // 32-bit counters
  ClaheParams q = p;
  clahe_constants(p.rows, p.cols, p.tiles_x, p.tiles_y, 0.0, q);
  if (q.tw != p.tw || q.th != p.th || q.scale != p.scale || q.inv_tw != p.inv_tw || q.inv_th != p.inv_th) return false;
  return p.clip >= 0 && (long long)p.clip <= (long long)p.tw * p.th;
}

// rows of a strip: kClaheStripRows, or as many as keep (tiles_y + 1) x strips below the grid's 65535
inline int clahe_strip_rows(const ClaheParams& p) {
  int rows = kClaheStripRows;
  while ((long long)(p.tiles_y + 1) * (p.th / rows + 1) > 65535) rows *= 2;
  return rows;
}

}  // namespace rip
