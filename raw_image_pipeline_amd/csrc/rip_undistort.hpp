// rip_undistort.hpp -- undistortion on the host: the new camera matrix and the maps of the fisheye and the pinhole models, and the
// compiler of the remap plan and of its footprint in the source image.
#pragma once
#include "rip_tile.hpp"

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace rip {

// ---------------------------------------------------------------------------------------------
// Fisheye undistortion (undistortion.cpp:197-238 -> OpenCV 4.2 calib3d/fisheye.cpp), double
// ---------------------------------------------------------------------------------------------
void fisheye_estimate_new_camera_matrix(const double K[9], const double D[4], int w, int h, const double R[9],
                                        double balance, int new_w, int new_h, double fov_scale, double newK[9]);
// Interleaved float2 map (x,y per destination pixel), w*h*2 floats.
// iR = (P R)^-1 of initUndistortRectifyMap (adjugate inverse), shared by the host builder and the device kernel
void fisheye_inverse_PR(const double P[9], const double R[9], double iR_out[9]);
void fisheye_init_undistort_rectify_map(const double K[9], const double D[4], const double R[9],
                                        const double P[9], int w, int h, float* map_xy);

// ---------------------------------------------------------------------------------------------
// Pinhole undistortion (distortion models plumb_bob, radtan, rational_polynomial: cv::getOptimalNewCameraMatrix and
// cv::initUndistortRectifyMap restated in double, PARITY.md "Pinhole distortion models"); not in the reference, which
// builds fisheye maps whatever the model says
// ---------------------------------------------------------------------------------------------
bool is_pinhole_model(const std::string& model);
// the length of the coefficient vector a model reports: 5 for plumb_bob and radtan, 8 for rational_polynomial, 4 otherwise
int distortion_coefficient_count(const std::string& model);
// the coefficients a pinhole model evaluates, (k1 k2 p1 p2 k3 k4 k5 k6): radtan takes k3 = 0, only rational_polynomial keeps k4..k6
void pinhole_coefficients(const std::string& model, const double D[8], double k[8]);
// alpha = balance clamped to [0, 1]: 0 crops to valid pixels, 1 keeps every source pixel.  Never throws.
void pinhole_estimate_new_camera_matrix(const double K[9], const double k[8], int w, int h, double balance, int new_w,
                                        int new_h, double fov_scale, double newK[9]);
// Interleaved float2 map like the fisheye one; iR = fisheye_inverse_PR(P, R)
void pinhole_init_undistort_rectify_map(const double K[9], const double k[8], const double R[9], const double P[9], int w,
                                        int h, float* map_xy);

// ---------------------------------------------------------------------------------------------
// Compiled remap plan.  cv::remap(INTER_LINEAR) quantises every map entry to 1/32 px before
// interpolating; the plan stores exactly that quantised form, organised in destination tiles of
// kRemapTileW x kRemapTileH pixels whose source footprint (a rectangle) is staged in LDS by the
// kernel.  Per destination pixel one 32-bit word: relx | rely << 11 | fx << 22 | fy << 27 with
// (relx, rely) relative to the tile's source rectangle; kRemapOutside: the pixel maps entirely
// outside the source (border constant 0); kRemapBorder: some taps fall outside -- the kernel
// takes the per-tap path on the float map for it.
// ---------------------------------------------------------------------------------------------
// kRemapTileW, kRemapTileH: rip_tile.hpp
constexpr uint32_t kRemapOutside = 0xFFFFFFFFu, kRemapBorder = 0xFFFFFFFEu;
struct RemapTile {
  int x0, y0, w, h;  // source rectangle in pixels (w == 0: no interior pixel in this tile)
};
struct RemapPlan {
  int drows = 0, dcols = 0, src_rows = 0, src_cols = 0;
  int tiles_x = 0, tiles_y = 0;
  std::vector<uint32_t> words;   // tile-major: tile t occupies words[t*1024 .. t*1024+1023], row-major inside
  std::vector<RemapTile> tiles;
  std::vector<uint32_t> border;  // (y << 16 | x) of every destination pixel marked kRemapBorder
  int max_rect_w = 0, max_rect_h = 0;
  size_t max_lds_bytes = 0;      // over tiles, for a source pixel size of 3 bytes
  // Footprint in the source image: per source row pair (rows 2i, 2i + 1) the hull [fp_lo[i], fp_hi[i]) of the 4-pixel groups
  // that hold a bilinear tap of some destination pixel -- interior and border pixels alike, from the same quantised
  // coordinates as the words; fp_lo[i] >= fp_hi[i]: no tap in that pair.  Filled by compile_remap_plan, or read back from
  // the device compiler (rip_maps.hip remap_footprint_kernel).
  std::vector<int> fp_lo, fp_hi;
  bool valid = false;
};
// LDS bytes the kernel needs for a source rectangle w x h of 3-byte pixels
size_t remap_tile_lds_bytes(int x0, int w, int h);
void compile_remap_plan(RemapPlan& plan, const float* map_xy, int drows, int dcols, int src_rows, int src_cols);
// The footprint part of compile_remap_plan on its own (lo / hi get (src_rows + 1) / 2 entries).
void compile_remap_footprint(const float* map_xy, int drows, int dcols, int src_rows, int src_cols, std::vector<int>& lo,
                             std::vector<int>& hi);
// The items of the fused Bayer chain kernel (pair << 16 | grp: the 4 x 2 pixels at source rows 2 pair, 2 pair + 1 and columns
// 4 grp .. 4 grp + 3 of its input, row-major) whose output lies in the footprint, for a chain of rows x cols pixels that
// writes the remap's source image flipped by flip_angle (0 or 180): item (pair, grp) writes row pair rows / 2 - 1 - pair and
// group cols / 4 - 1 - grp under the 180-degree flip.  rows even, cols a multiple of 4, rows / 2 <= 65535 and cols / 4 <= 65535
// (each index fills 16 bits: up to 131070 rows and 262140 columns; the callers -- rip_batch.cpp plan_route,
// rip_debug_chain_footprint -- walk densely or refuse past that).
void chain_footprint_items(const std::vector<int>& lo, const std::vector<int>& hi, int rows, int cols, int flip_angle,
                           std::vector<uint32_t>& items);

}  // namespace rip
