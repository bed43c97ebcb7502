// rip_clahe.hpp -- contrast-limited adaptive histogram equalisation of a delivered one-channel picture (rip_set_output_clahe;
// PARITY.md "Local contrast: CLAHE"): OpenCV 4's CLAHE_Impl::apply for CV_8UC1, restated.  Two kernels in a library of their own,
// librip_clahe_hip.so (rip_clahe.hip; device code rip_clahe_dev.hpp): clahe_lut_kernel makes one 256-byte table per (tile, frame),
// clahe_apply_kernel blends four tables per pixel.  This header is the library's whole interface -- plain data, the host's
// constants and two launch functions, which rip_output_stage.cpp calls at the end of a head's launches.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rip_launch_info.hpp"

namespace rip {

constexpr int kClaheBlock = 256;          // lanes of a workgroup of either kernel
constexpr int kClaheMaxTiles = 16;        // tiles per axis
constexpr int kClaheBins = 256;
constexpr int kClaheStripRows = 8;        // rows of the picture one workgroup of the apply kernel owns, inside one band
constexpr int kClaheLutLdsBytes = 4 * kClaheBins * 4;  // clahe_lut_kernel: one histogram per wave

struct ClaheParams {
  // the picture P, rows x cols pixels of one byte: src / dst point at its pixel (0, 0), at any byte alignment; rows `step` bytes and
  // frames `frame_stride` bytes apart.  dst may be src (in place): a lane reads its pixels before it writes them.  Only cols bytes of
  // a row are read or written.
  const uint8_t* src;
  size_t src_step, src_frame_stride;
  uint8_t* dst;
  size_t dst_step, dst_frame_stride;
  // the tables: n_frames x tiles_y x tiles_x x 256 bytes, 4-byte aligned; written by clahe_lut_kernel, read by clahe_apply_kernel
  uint8_t* lut;
  int rows, cols, n_frames;
  int tiles_x, tiles_y;
  int tw, th;       // the tile of the extended picture E (clahe_constants)
  int clip;         // cl; 0: no clipping
  float scale;      // 255.0f / (float)(tw * th)
  float inv_tw, inv_th;
};

// The constants of the definition (PARITY.md "Local contrast: CLAHE", steps 1 and 2) for a rows x cols picture: fills tiles_x,
// tiles_y, tw, th, clip, scale, inv_tw and inv_th of `p`.  Host arithmetic: float32 divisions, the clip in double.
inline void clahe_constants(int rows, int cols, int tiles_x, int tiles_y, double clip_limit, ClaheParams& p) {
  int erows = rows, ecols = cols;
  if (cols % tiles_x != 0 || rows % tiles_y != 0) {  // both axes grow as soon as one does not divide
    ecols = cols + tiles_x - cols % tiles_x;
    erows = rows + tiles_y - rows % tiles_y;
  }
  p.tiles_x = tiles_x;
  p.tiles_y = tiles_y;
  p.tw = ecols / tiles_x;
  p.th = erows / tiles_y;
  const int area = p.tw * p.th;
  p.scale = 255.0f / (float)area;
  p.inv_tw = 1.0f / (float)p.tw;
  p.inv_th = 1.0f / (float)p.th;
  p.clip = 0;
  if (clip_limit > 0) {
    double c = clip_limit * area / 256;
    if (c > (double)area) c = (double)area;
    p.clip = (int)c > 1 ? (int)c : 1;
  }
}

// bytes of the tables of n frames
inline size_t clahe_lut_bytes(int tiles_x, int tiles_y, int n_frames) { return (size_t)n_frames * tiles_x * tiles_y * kClaheBins; }

// Enqueue the table kernel / the blend of n_frames frames on `stream`.  false -- nothing launched -- for a null pointer, a picture
// with fewer than two pixels per tile and side, tile counts outside 1 .. kClaheMaxTiles, constants that are not clahe_constants' of
// that picture, a pitch below a row, a misaligned table block or a frame count outside 1 .. 65535.
__attribute__((visibility("default"))) bool launch_clahe_lut(const ClaheParams& p, hipStream_t stream, LaunchInfo* info);
__attribute__((visibility("default"))) bool launch_clahe_apply(const ClaheParams& p, hipStream_t stream, LaunchInfo* info);

}  // namespace rip
