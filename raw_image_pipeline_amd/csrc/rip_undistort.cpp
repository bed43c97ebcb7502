// rip_undistort.cpp -- fisheye and pinhole map construction, remap plan and footprint compiler (rip_undistort.hpp).
// Float expressions here define bit patterns the kernels depend on: compile with -ffp-contract=off (build.py does).
#include "rip_undistort.hpp"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <thread>

namespace rip {

// ---------------------------------------------------------------------------------------------
// Fisheye
// ---------------------------------------------------------------------------------------------
namespace {
struct Mat3 {
  double v[9];
};
Mat3 mul3(const double* a, const double* b) {
  Mat3 c;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) c.v[i * 3 + j] = a[i * 3 + 0] * b[0 * 3 + j] + a[i * 3 + 1] * b[1 * 3 + j] + a[i * 3 + 2] * b[2 * 3 + j];
  return c;
}
Mat3 inverse3(const Mat3& m) {
  const double* a = m.v;
  double c0 = a[4] * a[8] - a[5] * a[7];
  double c1 = a[5] * a[6] - a[3] * a[8];
  double c2 = a[3] * a[7] - a[4] * a[6];
  double inv_det = 1.0 / (a[0] * c0 + a[1] * c1 + a[2] * c2);
  Mat3 o;
  o.v[0] = c0 * inv_det;
  o.v[1] = (a[2] * a[7] - a[1] * a[8]) * inv_det;
  o.v[2] = (a[1] * a[5] - a[2] * a[4]) * inv_det;
  o.v[3] = c1 * inv_det;
  o.v[4] = (a[0] * a[8] - a[2] * a[6]) * inv_det;
  o.v[5] = (a[2] * a[3] - a[0] * a[5]) * inv_det;
  o.v[6] = c2 * inv_det;
  o.v[7] = (a[1] * a[6] - a[0] * a[7]) * inv_det;
  o.v[8] = (a[0] * a[4] - a[1] * a[3]) * inv_det;
  return o;
}

// cv::fisheye::undistortPoints for one point (Newton iteration on theta, <= 10 steps)
void undistort_point(const double K[9], const double D[4], const double R[9], double u, double v, double& ox, double& oy) {
  const double pi = 3.1415926535897932384626433832795;
  double wx = (u - K[2]) / K[0], wy = (v - K[5]) / K[4];
  double theta_d = std::sqrt(wx * wx + wy * wy);
  theta_d = std::min(std::max(-pi / 2., theta_d), pi / 2.);
  double scale = 1.0;
  if (theta_d > 1e-8) {
    double theta = theta_d;
    for (int it = 0; it < 10; it++) {
      double t2 = theta * theta, t4 = t2 * t2, t6 = t4 * t2, t8 = t6 * t2;
      double a = D[0] * t2, b = D[1] * t4, c = D[2] * t6, d = D[3] * t8;
      double fix = (theta * (1 + a + b + c + d) - theta_d) / (1 + 3 * a + 5 * b + 7 * c + 9 * d);
      theta = theta - fix;
      if (std::fabs(fix) < 1e-8) break;
    }
    scale = std::tan(theta) / theta_d;
  }
  double ux = wx * scale, uy = wy * scale;
  double rx = R[0] * ux + R[1] * uy + R[2];
  double ry = R[3] * ux + R[4] * uy + R[5];
  double rz = R[6] * ux + R[7] * uy + R[8];
  ox = rx / rz;
  oy = ry / rz;
}
}  // namespace

void fisheye_estimate_new_camera_matrix(const double K[9], const double D[4], int w, int h, const double R[9],
                                        double balance, int new_w, int new_h, double fov_scale, double newK[9]) {
  balance = std::min(std::max(balance, 0.0), 1.0);
  // mid-points of the four image edges, integer halves as in OpenCV
  const double px[4] = {(double)(w / 2), (double)w, (double)(w / 2), 0.0};
  const double py[4] = {0.0, (double)(h / 2), (double)h, (double)(h / 2)};
  double ux[4], uy[4];
  for (int i = 0; i < 4; i++) undistort_point(K, D, R, px[i], py[i], ux[i], uy[i]);
  double cx = (ux[0] + ux[1] + ux[2] + ux[3]) / 4, cy = (uy[0] + uy[1] + uy[2] + uy[3]) / 4;
  double aspect = K[0] / K[4];
  cx *= aspect;  // OpenCV 4.2 scales cn[0] here (later releases scale cn[1]); kept as in 4.2
  for (int i = 0; i < 4; i++) uy[i] *= aspect;
  double minx = DBL_MAX, miny = DBL_MAX, maxx = -DBL_MAX, maxy = -DBL_MAX;
  for (int i = 0; i < 4; i++) {
    miny = std::min(miny, uy[i]);
    maxy = std::max(maxy, uy[i]);
    minx = std::min(minx, ux[i]);
    maxx = std::max(maxx, ux[i]);
  }
  double f1 = w * 0.5 / (cx - minx), f2 = w * 0.5 / (maxx - cx);
  double f3 = h * 0.5 * aspect / (cy - miny), f4 = h * 0.5 * aspect / (maxy - cy);
  double fmin = std::min(f1, std::min(f2, std::min(f3, f4)));
  double fmax = std::max(f1, std::max(f2, std::max(f3, f4)));
  double f = balance * fmin + (1.0 - balance) * fmax;
  f *= fov_scale > 0 ? 1.0 / fov_scale : 1.0;
  double fx = f, fy = f;
  double ncx = -cx * f + w * 0.5, ncy = -cy * f + (h * aspect) * 0.5;
  fy /= aspect;
  ncy /= aspect;
  if (new_w > 0 && new_h > 0) {
    double rx = new_w / (double)w, ry = new_h / (double)h;
    fx *= rx;
    fy *= ry;
    ncx *= rx;
    ncy *= ry;
  }
  const double out[9] = {fx, 0, ncx, 0, fy, ncy, 0, 0, 1};
  std::memcpy(newK, out, sizeof(out));
}

void fisheye_inverse_PR(const double P[9], const double R[9], double iR_out[9]) {
  const Mat3 iR = inverse3(mul3(P, R));
  for (int i = 0; i < 9; i++) iR_out[i] = iR.v[i];
}

namespace {
// rows [0, h) of a w x h map on up to 16 threads; small maps on the caller's
template <typename RowsFn>
void for_map_rows(int w, int h, const RowsFn& rows_fn) {
  int nthreads = (int)std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u);
  if ((size_t)w * h < (1u << 18) || nthreads == 1) {
    rows_fn(0, h);
    return;
  }
  std::vector<std::thread> pool;
  int chunk = (h + nthreads - 1) / nthreads;
  for (int t = 0; t < nthreads; t++) {
    int r0 = t * chunk, r1 = std::min(h, r0 + chunk);
    if (r0 < r1) pool.emplace_back(rows_fn, r0, r1);
  }
  for (auto& th : pool) th.join();
}
}  // namespace

void fisheye_init_undistort_rectify_map(const double K[9], const double D[4], const double R[9],
                                        const double P[9], int w, int h, float* map_xy) {
  Mat3 iR = inverse3(mul3(P, R));
  const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  auto rows_fn = [&](int r0, int r1) {
    for (int i = r0; i < r1; i++) {
      double X = i * iR.v[1] + iR.v[2], Y = i * iR.v[4] + iR.v[5], W = i * iR.v[7] + iR.v[8];
      float* out = map_xy + (size_t)i * w * 2;
      for (int j = 0; j < w; j++) {
        double x = X / W, y = Y / W;
        double r = std::sqrt(x * x + y * y);
        double theta = std::atan(r);
        double t2 = theta * theta, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
        double theta_d = theta * (1 + D[0] * t2 + D[1] * t4 + D[2] * t6 + D[3] * t8);
        double s = (r == 0) ? 1.0 : theta_d / r;
        out[2 * j] = (float)(fx * x * s + cx);
        out[2 * j + 1] = (float)(fy * y * s + cy);
        X += iR.v[0];  // accumulated along the row, as OpenCV does
        Y += iR.v[3];
        W += iR.v[6];
      }
    }
  };
  for_map_rows(w, h, rows_fn);
}

// ---------------------------------------------------------------------------------------------
// Pinhole models (plumb_bob, radtan, rational_polynomial)
// ---------------------------------------------------------------------------------------------
bool is_pinhole_model(const std::string& model) {
  return model == "plumb_bob" || model == "radtan" || model == "rational_polynomial";
}

int distortion_coefficient_count(const std::string& model) {
  if (model == "rational_polynomial") return 8;
  return is_pinhole_model(model) ? 5 : 4;
}

void pinhole_coefficients(const std::string& model, const double D[8], double k[8]) {
  const int n = model == "rational_polynomial" ? 8 : model == "plumb_bob" ? 5 : 4;
  for (int i = 0; i < 8; i++) k[i] = i < n ? D[i] : 0.0;
}

// cv::getOptimalNewCameraMatrix: a 9 x 9 grid of source points is undistorted (20 fixed-point iterations, no R); the
// inner rectangle holds only valid pixels, the outer one every source pixel, and balance blends the two cameras
void pinhole_estimate_new_camera_matrix(const double K[9], const double k[8], int w, int h, double balance, int new_w,
                                        int new_h, double fov_scale, double newK[9]) {
  balance = std::min(std::max(balance, 0.0), 1.0);
  const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
  constexpr int N = 9;
  double px[N][N], py[N][N];
  for (int gy = 0; gy < N; gy++)
    for (int gx = 0; gx < N; gx++) {
      const double u = gx * (double)(w - 1) / 8, v = gy * (double)(h - 1) / 8;
      const double x0 = (u - K[2]) / K[0], y0 = (v - K[5]) / K[4];
      double x = x0, y = y0;
      for (int it = 0; it < 20; it++) {
        const double r2 = x * x + y * y;
        const double icd = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2);
        const double dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
        const double dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
        x = (x0 - dx) * icd;
        y = (y0 - dy) * icd;
      }
      px[gy][gx] = x;
      py[gy][gx] = y;
    }
  double il = -DBL_MAX, ir = DBL_MAX, it_ = -DBL_MAX, ib = DBL_MAX;  // inner: left, right, top, bottom
  double ol = DBL_MAX, or_ = -DBL_MAX, ot = DBL_MAX, ob = -DBL_MAX;  // outer
  for (int a = 0; a < N; a++) {
    il = std::max(il, px[a][0]);
    ir = std::min(ir, px[a][N - 1]);
    it_ = std::max(it_, py[0][a]);
    ib = std::min(ib, py[N - 1][a]);
    for (int b = 0; b < N; b++) {
      ol = std::min(ol, px[a][b]);
      or_ = std::max(or_, px[a][b]);
      ot = std::min(ot, py[a][b]);
      ob = std::max(ob, py[a][b]);
    }
  }
  const double nw = new_w, nh = new_h;
  const double fx0 = (nw - 1) / (ir - il), fy0 = (nh - 1) / (ib - it_), cx0 = -fx0 * il, cy0 = -fy0 * it_;
  const double fx1 = (nw - 1) / (or_ - ol), fy1 = (nh - 1) / (ob - ot), cx1 = -fx1 * ol, cy1 = -fy1 * ot;
  double fx = fx0 * (1 - balance) + fx1 * balance, fy = fy0 * (1 - balance) + fy1 * balance;
  const double cx = cx0 * (1 - balance) + cx1 * balance, cy = cy0 * (1 - balance) + cy1 * balance;
  if (fov_scale > 0) {
    fx = fx / fov_scale;
    fy = fy / fov_scale;
  }
  const double out[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
  std::memcpy(newK, out, sizeof(out));
}

// cv::initUndistortRectifyMap (CV_32FC1) in double, statement for statement what rip_maps.hip pinhole_maps_kernel does
void pinhole_init_undistort_rectify_map(const double K[9], const double k[8], const double R[9], const double P[9], int w,
                                        int h, float* map_xy) {
  const Mat3 iR = inverse3(mul3(P, R));
  const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
  auto rows_fn = [&](int r0, int r1) {
    for (int i = r0; i < r1; i++) {
      double X = i * iR.v[1] + iR.v[2], Y = i * iR.v[4] + iR.v[5], W = i * iR.v[7] + iR.v[8];
      float* out = map_xy + (size_t)i * w * 2;
      for (int j = 0; j < w; j++) {
        const double wi = 1.0 / W, x = X * wi, y = Y * wi;
        const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2 * x * y;
        const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
        const double xd = x * kr + p1 * xy2 + p2 * (r2 + 2 * x2);
        const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * xy2;
        out[2 * j] = (float)(fx * xd + cx);
        out[2 * j + 1] = (float)(fy * yd + cy);
        X += iR.v[0];  // accumulated along the row, as OpenCV does
        Y += iR.v[3];
        W += iR.v[6];
      }
    }
  };
  for_map_rows(w, h, rows_fn);
}

// ---------------------------------------------------------------------------------------------
// Compiled remap plan
// ---------------------------------------------------------------------------------------------
namespace {
inline int quantise_map(float v) {
  // cvRound(v * INTER_TAB_SIZE) as cv::remap does (imgwarp.cpp); INT_MIN for NaN / inf / overflow
  float s = v * 32.f;
  if (!(s > -2147483648.f && s < 2147483648.f)) return INT32_MIN;
  return (int)std::lrintf(s);
}
inline int sat_s16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
}  // namespace

size_t remap_tile_lds_bytes(int x0, int w, int h) {
  if (w <= 0 || h <= 0) return 0;
  // rows start at the 16-byte chunk that holds byte 3 * x0 and end with the chunk that holds the last byte
  size_t pitch = ((((size_t)x0 * 3) & 15) + (size_t)w * 3 + 15) & ~(size_t)15;
  return pitch * (size_t)h;
}

void compile_remap_footprint(const float* map_xy, int drows, int dcols, int src_rows, int src_cols, std::vector<int>& lo,
                             std::vector<int>& hi) {
  const int pairs = (src_rows + 1) / 2;
  lo.assign(pairs, INT32_MAX);
  hi.assign(pairs, 0);
  for (int y = 0; y < drows; y++)
    for (int x = 0; x < dcols; x++) {
      const float* m = map_xy + ((size_t)y * dcols + x) * 2;
      const int sx = sat_s16(quantise_map(m[0]) >> 5), sy = sat_s16(quantise_map(m[1]) >> 5);
      // the in-bounds taps of {sx, sx + 1} x {sy, sy + 1}: what the interior word or the per-tap border path reads
      const int x0 = std::max(sx, 0), x1 = std::min(sx + 1, src_cols - 1);
      const int y0 = std::max(sy, 0), y1 = std::min(sy + 1, src_rows - 1);
      if (x0 > x1 || y0 > y1) continue;  // outside: no tap
      for (int r = y0; r <= y1; r++) {
        const int i = r >> 1;
        lo[i] = std::min(lo[i], x0 >> 2);
        hi[i] = std::max(hi[i], (x1 >> 2) + 1);
      }
    }
}

void chain_footprint_items(const std::vector<int>& lo, const std::vector<int>& hi, int rows, int cols, int flip_angle,
                           std::vector<uint32_t>& items) {
  items.clear();
  const int pairs = rows / 2, groups = cols / 4;
  const bool flip180 = flip_angle == 180;
  for (int pair = 0; pair < pairs; pair++) {
    const int fp = flip180 ? pairs - 1 - pair : pair;  // the row pair of the remap's source image this item writes
    if (fp >= (int)lo.size() || lo[fp] >= hi[fp]) continue;
    const int g_lo = std::max(0, flip180 ? groups - hi[fp] : lo[fp]);
    const int g_hi = std::min(groups, flip180 ? groups - lo[fp] : hi[fp]);
    for (int g = g_lo; g < g_hi; g++) items.push_back(((uint32_t)pair << 16) | (uint32_t)g);
  }
}

void compile_remap_plan(RemapPlan& plan, const float* map_xy, int drows, int dcols, int src_rows, int src_cols) {
  plan = RemapPlan();
  plan.drows = drows;
  plan.dcols = dcols;
  plan.src_rows = src_rows;
  plan.src_cols = src_cols;
  plan.tiles_x = (dcols + kRemapTileW - 1) / kRemapTileW;
  plan.tiles_y = (drows + kRemapTileH - 1) / kRemapTileH;
  const size_t ntiles = (size_t)plan.tiles_x * plan.tiles_y;
  const int tile_px = kRemapTileW * kRemapTileH;
  plan.words.assign(ntiles * tile_px, kRemapOutside);
  plan.tiles.assign(ntiles, RemapTile{0, 0, 0, 0});
  auto do_tiles = [&](size_t t0, size_t t1) {
    std::vector<int> ix(tile_px), iy(tile_px);
    for (size_t t = t0; t < t1; t++) {
      const int ty = (int)(t / plan.tiles_x), tx = (int)(t % plan.tiles_x);
      int minx = INT32_MAX, miny = INT32_MAX, maxx = INT32_MIN, maxy = INT32_MIN;
      uint32_t* words = plan.words.data() + t * tile_px;
      for (int r = 0; r < kRemapTileH; r++)
        for (int c = 0; c < kRemapTileW; c++) {
          const int y = ty * kRemapTileH + r, x = tx * kRemapTileW + c, k = r * kRemapTileW + c;
          if (y >= drows || x >= dcols) {
            words[k] = kRemapOutside;  // never stored
            ix[k] = INT32_MIN;
            continue;
          }
          const float* m = map_xy + ((size_t)y * dcols + x) * 2;
          const int sxq = quantise_map(m[0]), syq = quantise_map(m[1]);
          const int sx = sat_s16(sxq >> 5), sy = sat_s16(syq >> 5);
          if (sx >= src_cols || sx + 1 < 0 || sy >= src_rows || sy + 1 < 0) {
            words[k] = kRemapOutside;
            ix[k] = INT32_MIN;
          } else if (sx >= 0 && sx < src_cols - 1 && sy >= 0 && sy < src_rows - 1) {
            words[k] = ((uint32_t)(sxq & 31) << 22) | ((uint32_t)(syq & 31) << 27);  // rel coords filled below
            ix[k] = sx;
            iy[k] = sy;
            minx = std::min(minx, sx);
            maxx = std::max(maxx, sx + 1);
            miny = std::min(miny, sy);
            maxy = std::max(maxy, sy + 1);
          } else {
            words[k] = kRemapBorder;
            ix[k] = INT32_MIN;
          }
        }
      RemapTile& tile = plan.tiles[t];
      if (minx == INT32_MAX) continue;
      tile.x0 = minx;
      tile.y0 = miny;
      tile.w = maxx - minx + 1;
      tile.h = maxy - miny + 1;
      if (tile.w > 2040 || tile.h > 2040) {
        // footprint too large for the packed form: everything in this tile takes the per-tap path
        for (int k = 0; k < tile_px; k++)
          if (ix[k] != INT32_MIN) words[k] = kRemapBorder;
        tile = RemapTile{0, 0, 0, 0};
        continue;
      }
      for (int k = 0; k < tile_px; k++)
        if (ix[k] != INT32_MIN) words[k] |= (uint32_t)(ix[k] - minx) | ((uint32_t)(iy[k] - miny) << 11);
    }
  };
  int nthreads = (int)std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u);
  if (ntiles < 64 || nthreads == 1) {
    do_tiles(0, ntiles);
  } else {
    std::vector<std::thread> pool;
    size_t chunk = (ntiles + nthreads - 1) / nthreads;
    for (int i = 0; i < nthreads; i++) {
      size_t a = i * chunk, b = std::min(ntiles, a + chunk);
      if (a < b) pool.emplace_back(do_tiles, a, b);
    }
    for (auto& th : pool) th.join();
  }
  if (drows <= 65535 && dcols <= 65535) {
    for (size_t t = 0; t < ntiles; t++) {
      const int ty = (int)(t / plan.tiles_x), tx = (int)(t % plan.tiles_x);
      const uint32_t* words = plan.words.data() + t * tile_px;
      for (int k = 0; k < tile_px; k++)
        if (words[k] == kRemapBorder) {
          const int y = ty * kRemapTileH + k / kRemapTileW, x = tx * kRemapTileW + k % kRemapTileW;
          if (y < drows && x < dcols) plan.border.push_back(((uint32_t)y << 16) | (uint32_t)x);
        }
    }
  }
  compile_remap_footprint(map_xy, drows, dcols, src_rows, src_cols, plan.fp_lo, plan.fp_hi);
  for (const RemapTile& tile : plan.tiles) {
    plan.max_rect_w = std::max(plan.max_rect_w, tile.w);
    plan.max_rect_h = std::max(plan.max_rect_h, tile.h);
    plan.max_lds_bytes = std::max(plan.max_lds_bytes, remap_tile_lds_bytes(tile.x0, tile.w, tile.h));
  }
  plan.valid = true;
}

}  // namespace rip
