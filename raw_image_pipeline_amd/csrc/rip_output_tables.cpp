// rip_output_tables.cpp -- the tables of the output and resize stage (rip_output_tables.hpp).
// Float expressions here define bit patterns the kernels depend on: compile with -ffp-contract=off (build.py does).
#include "rip_output_tables.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace rip {

namespace {
// index = the id output_yuv_matrix_id returns; the rows are rip_yuv.hpp's YuvMatrix (PARITY.md "Output formats: YUV 4:2:0")
const int kYuvMatrices[4][10] = {
    {3208, 16520, 8414, 14392, -9535, -4857, -2341, -12051, 14392, 16},
    {2032, 20127, 5983, 14392, -11094, -3298, -1320, -13072, 14392, 16},
    {3735, 19235, 9798, 16384, -10855, -5529, -2664, -13720, 16384, 0},
    {2366, 23436, 6966, 16384, -12630, -3754, -1502, -14882, 16384, 0}};

uint32_t float_bits(float f) {
  uint32_t x;
  std::memcpy(&x, &f, sizeof(x));
  return x;
}
// IEEE 754 binary32 -> binary16, round to nearest even
uint16_t f32_to_f16(float f) {
  uint32_t x = float_bits(f);
  const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
  x &= 0x7FFFFFFFu;
  if (x > 0x7F800000u) return (uint16_t)(sign | 0x7E00u);  // NaN
  const int e = (int)(x >> 23);
  uint32_t m = x & 0x7FFFFFu;
  if (e >= 143) return (uint16_t)(sign | 0x7C00u);  // 2^16 and above, inf
  if (e >= 113) {                                    // normal halves; a carry out of the mantissa goes into the exponent, up to inf
    uint32_t h = ((uint32_t)(e - 112) << 10) | (m >> 13);
    const uint32_t rem = m & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;
    return (uint16_t)(sign | h);
  }
  if (e < 102) return sign;  // below 2^-25: zero
  m |= 0x800000u;            // subnormal halves, in units of 2^-24
  const int shift = 126 - e;
  uint32_t h = m >> shift;
  const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
  if (rem > half || (rem == half && (h & 1u))) h++;
  return (uint16_t)(sign | h);
}
// binary32 -> bfloat16, round to nearest even
uint16_t f32_to_bf16(float f) {
  const uint32_t x = float_bits(f);
  if ((x & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((x >> 16) | 0x0040u);  // NaN stays NaN
  return (uint16_t)((x + 0x7FFFu + ((x >> 16) & 1u)) >> 16);
}
}  // namespace

void output_yuv_matrix(int id, int coef[9], int* yoff) {
  if (id < 0 || id > 3) throw std::invalid_argument("no such YUV matrix");
  for (int i = 0; i < 9; i++) coef[i] = kYuvMatrices[id][i];
  *yoff = kYuvMatrices[id][9];
}

void check_output_normalization(double divisor, const double mean[3], const double sd[3]) {
  bool ok = std::isfinite(divisor) && divisor != 0.0;
  for (int i = 0; i < 3 && ok; i++) ok = std::isfinite(mean[i]) && std::isfinite(sd[i]) && sd[i] != 0.0;
  if (!ok) throw std::invalid_argument("output normalisation: divisor, mean and std must be finite, divisor and every std non-zero");
}

void build_output_table(int format, double divisor, const double mean[3], const double sd[3], void* out) {
  if (format < 3 || format > 8) throw std::invalid_argument("this output format has no table (the planar float formats have one)");
  check_output_normalization(divisor, mean, sd);
  const int kind = (format - 3) % 3;  // f32, f16, bf16
  for (int c = 0; c < 3; c++)
    for (int v = 0; v < 256; v++) {
      volatile double q = (double)v / divisor;  // every operation rounded to double on its own
      volatile double d = q - mean[c];
      const float t = (float)(d / sd[c]);
      const int i = c * 256 + v;
      if (kind == 0) static_cast<float*>(out)[i] = t;
      else static_cast<uint16_t*>(out)[i] = kind == 1 ? f32_to_f16(t) : f32_to_bf16(t);
    }
}

void build_resize_tables(int R, int C, int H, int W, int32_t* xofs, int16_t* alpha, int32_t* yofs, int16_t* beta, int* area2) {
  for (int side : {R, C, H, W})
    if (side < 1 || side > 16384) throw std::invalid_argument("resize: every side of the source and of the target must be in 1..16384");
  if (!xofs || !alpha || !yofs || !beta) throw std::invalid_argument("resize: null table");
  fill_resize_tables(R, C, H, W, xofs, alpha, yofs, beta);
  if (area2) *area2 = (R == 2 * H && C == 2 * W) ? 1 : 0;
}

void fill_resize_tables(int R, int C, int H, int W, int32_t* xofs, int16_t* alpha, int32_t* yofs, int16_t* beta) {
  // imgproc/resize.cpp, the statements of oracle/rip_oracle.c ripo_resize_linear_8u; weights beyond 16 bits cannot occur (f in [0, 1))
  const double scale_x = (double)C / W, scale_y = (double)R / H;
  for (int dx = 0; dx < W; dx++) {
    float fx = (float)((dx + 0.5) * scale_x - 0.5);
    int sx = (int)std::floor(fx);
    fx -= sx;
    if (sx < 0) { fx = 0; sx = 0; }
    if (sx >= C - 1) { fx = 0; sx = C - 1; }
    xofs[dx] = sx;
    alpha[2 * dx] = (int16_t)std::lrintf((1.f - fx) * 2048);
    alpha[2 * dx + 1] = (int16_t)std::lrintf(fx * 2048);
  }
  for (int dy = 0; dy < H; dy++) {
    float fy = (float)((dy + 0.5) * scale_y - 0.5);
    const int sy = (int)std::floor(fy);
    fy -= sy;
    beta[2 * dy] = (int16_t)std::lrintf((1.f - fy) * 2048);
    beta[2 * dy + 1] = (int16_t)std::lrintf(fy * 2048);
    yofs[2 * dy] = std::min(std::max(sy, 0), R - 1);
    yofs[2 * dy + 1] = std::min(std::max(sy + 1, 0), R - 1);
  }
}

int output_pad_grey(int b, int g, int r) { return (3735 * b + 19235 * g + 9798 * r + 16384) >> 15; }

void output_window_geometry(int C, int R, const int roi[4], int W, int H, int fit, int src[4], int dst[4]) {
  int x = 0, y = 0, w = C, h = R;
  if (roi[2] > 0) {
    x = roi[0], y = roi[1], w = roi[2], h = roi[3];
    if (x > C - w || y > R - h)  // x + w > C or y + h > R, without the sum
      throw std::invalid_argument("output roi (" + std::to_string(x) + ", " + std::to_string(y) + ", " + std::to_string(w) + ", " + std::to_string(h) +
                                  ") does not lie inside the pipeline's image of " + std::to_string(C) + " x " + std::to_string(R));
  }
  const auto clamp = [](long long v, int lo, int hi) { return (int)std::min<long long>(std::max<long long>(v, lo), hi); };
  int left = 0, top = 0, wi = W > 0 ? W : w, hi = W > 0 ? H : h;
  if (W > 0 && fit == 2) {  // the centred sub-window with the target's aspect
    if ((long long)w * H >= (long long)h * W) {
      const int w2 = clamp((2ll * h * W + H) / (2ll * H), 1, w);
      x += (w - w2) / 2;
      w = w2;
    } else {
      const int h2 = clamp((2ll * w * H + W) / (2ll * W), 1, h);
      y += (h - h2) / 2;
      h = h2;
    }
  } else if (W > 0 && fit == 1) {  // the whole window, centred in the target
    if ((long long)W * h <= (long long)H * w) hi = clamp((2ll * h * W + w) / (2ll * w), 1, H);
    else wi = clamp((2ll * w * H + h) / (2ll * h), 1, W);
    left = (W - wi) / 2;
    top = (H - hi) / 2;
  }
  src[0] = x, src[1] = y, src[2] = w, src[3] = h;
  dst[0] = left, dst[1] = top, dst[2] = wi, dst[3] = hi;
}

void check_resize_area_sizes(int R, int C, int H, int W) {
  for (int side : {R, C, H, W})
    if (side < 1 || side > 16384) throw std::invalid_argument("resize: every side of the source and of the target must be in 1..16384");
  const std::string sizes = "from " + std::to_string(C) + " x " + std::to_string(R) + " to " + std::to_string(W) + " x " + std::to_string(H);
  if (W > C || H > R) throw std::invalid_argument("output interpolation \"area\" is a downscale filter: " + sizes + " enlarges an axis (use \"linear\")");
  if (C > 256 * W || R > 256 * H) throw std::invalid_argument("output interpolation \"area\" takes factors up to 256 per axis: " + sizes + " is beyond that");
}

size_t build_area_axis(int s, int d, int32_t* first, int32_t* count, float* weights) {
  const double scale = (double)s / d;
  size_t n = 0;
  for (int i = 0; i < d; i++) {
    const double f1 = i * scale, f2 = f1 + scale, cell = std::min(scale, s - f1);
    int s1 = (int)std::ceil(f1);
    const int s2 = std::min((int)std::floor(f2), s - 1);
    s1 = std::min(s1, s2);
    const size_t n0 = n;
    int lead = s1;  // the first source sample of this output
    if (s1 - f1 > 1e-3) {
      lead = s1 - 1;
      weights[n++] = (float)((s1 - f1) / cell);
    }
    for (int k = s1; k < s2; k++) weights[n++] = (float)(1.0 / cell);
    if (f2 - s2 > 1e-3) {
      if (n == n0) lead = s2;
      weights[n++] = (float)(std::min(std::min(f2 - s2, 1.0), cell) / cell);
    }
    first[i] = lead;
    count[i] = (int32_t)(n - n0);
  }
  return n;
}

void build_resize_area_tables(int R, int C, int H, int W, int32_t* xfirst, int32_t* xcount, float* xweight, int32_t* yfirst, int32_t* ycount,
                              float* yweight, int* whole, float* scale) {
  check_resize_area_sizes(R, C, H, W);
  if (!xfirst || !xcount || !xweight || !yfirst || !ycount || !yweight) throw std::invalid_argument("resize: null table");
  build_area_axis(C, W, xfirst, xcount, xweight);
  build_area_axis(R, H, yfirst, ycount, yweight);
  const bool is_whole = R % H == 0 && C % W == 0 && !(R == H && C == W) && !(R == 2 * H && C == 2 * W);
  if (whole) *whole = is_whole ? 1 : 0;
  if (scale) *scale = is_whole ? 1.f / (float)((R / H) * (C / W)) : 0.f;
}

void check_resize_aa_sizes(int R, int C, int H, int W) {
  for (int side : {R, C, H, W})
    if (side < 1 || side > 16384) throw std::invalid_argument("resize: every side of the source and of the target must be in 1..16384");
  if (C > 64 * W || R > 64 * H)
    throw std::invalid_argument("output interpolations \"linear_aa\" and \"cubic_aa\" take factors up to 64 per axis: from " + std::to_string(C) + " x " +
                                std::to_string(R) + " to " + std::to_string(W) + " x " + std::to_string(H) + " is beyond that");
}

namespace {
// the filters of PARITY.md "Resize: antialiased filters", in double
double aa_linear(double t) {
  t = std::fabs(t);
  return t < 1.0 ? 1.0 - t : 0.0;
}
double aa_cubic(double t) {
  const double a = -0.5;
  t = std::fabs(t);
  if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
  if (t < 2.0) return (((t - 5.0) * t + 8.0) * t - 4.0) * a;
  return 0.0;
}
int aa_support(int filter) {
  if (filter != 2 && filter != 3) throw std::invalid_argument("resize: the antialiased filters are 2 (linear_aa) and 3 (cubic_aa)");
  return filter == 3 ? 2 : 1;
}
}  // namespace

size_t resize_aa_weight_capacity(int filter, int s, int d) { return 2 * (size_t)aa_support(filter) * (size_t)std::max(s, d) + (size_t)d; }

size_t build_aa_axis(int filter, int s, int d, int32_t* first, int32_t* count, int32_t* wofs, int16_t* weights, int* prec) {
  const int S = aa_support(filter);
  const double scale = (double)s / d;
  const double support = scale >= 1.0 ? S * scale : (double)S;
  const double inv = scale >= 1.0 ? 1.0 / scale : 1.0;
  std::vector<double> w;
  w.reserve(resize_aa_weight_capacity(filter, s, d));
  double wmax = 0.0;
  for (int i = 0; i < d; i++) {
    const double c = scale * (i + 0.5);
    const int lo = std::max((int)(c - support + 0.5), 0);
    const int n = std::min((int)(c + support + 0.5), s) - lo;
    const size_t at = w.size();
    double t = 0.0;
    for (int j = 0; j < n; j++) {
      const double v = filter == 3 ? aa_cubic((j + lo - c + 0.5) * inv) : aa_linear((j + lo - c + 0.5) * inv);
      w.push_back(v);
      t += v;
    }
    for (size_t k = at; k < w.size(); k++) {
      if (t != 0.0) w[k] = w[k] / t;
      wmax = std::max(wmax, w[k]);
    }
    first[i] = lo;
    count[i] = n;
    if (wofs) wofs[i] = (int32_t)at;
  }
  int pr = 0;
  while (pr < 22 && (int)(0.5 + wmax * (double)(1 << (pr + 1))) < (1 << 15)) pr++;
  for (size_t k = 0; k < w.size(); k++)
    weights[k] = (int16_t)(w[k] >= 0.0 ? (int)(0.5 + w[k] * (double)(1 << pr)) : (int)(-0.5 + w[k] * (double)(1 << pr)));
  if (prec) *prec = pr;
  return w.size();
}

int aa_lds_rows(int s, int d, const int32_t* first, const int32_t* count, int th) {
  int span = 0;
  for (int y0 = 0; y0 < d; y0 += th) {
    const int y1 = std::min(d, y0 + th) - 1;
    span = std::max(span, s == d ? y1 - y0 + 1 : first[y1] + count[y1] - first[y0]);
  }
  return span;
}

int aa_tile_rows(int s, int d, const int32_t* first, const int32_t* count, int channels, int* lds_rows) {
  for (int th = 8; th >= 1; th /= 2) {
    const int span = aa_lds_rows(s, d, first, count, th);
    if ((size_t)span * 64 * (size_t)channels <= 65536 || th == 1) {
      if (lds_rows) *lds_rows = span;
      return th;
    }
  }
  return 1;
}

void build_resize_aa_tables(int filter, int R, int C, int H, int W, int32_t* xfirst, int32_t* xcount, int32_t* xwofs, int16_t* xweight, int* xprec,
                            int32_t* yfirst, int32_t* ycount, int32_t* ywofs, int16_t* yweight, int* yprec, int tile_rows[2], int lds_rows[2]) {
  (void)aa_support(filter);
  check_resize_aa_sizes(R, C, H, W);
  if (!xfirst || !xcount || !xweight || !yfirst || !ycount || !yweight) throw std::invalid_argument("resize: null table");
  build_aa_axis(filter, C, W, xfirst, xcount, xwofs, xweight, xprec);
  build_aa_axis(filter, R, H, yfirst, ycount, ywofs, yweight, yprec);
  for (int k = 0; k < 2; k++) {
    int rows = 0;
    const int th = aa_tile_rows(R, H, yfirst, ycount, k ? 3 : 1, &rows);
    if (tile_rows) tile_rows[k] = th;
    if (lds_rows) lds_rows[k] = rows;
  }
}

}  // namespace rip
