// rip_color_tables.cpp -- gamma, Lab / HSV and vignetting tables (rip_color_tables.hpp).
// Float expressions here define bit patterns the kernels depend on: compile with -ffp-contract=off (build.py does).
#include "rip_color_tables.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace rip {

// =============================================================================================
// Tables
// =============================================================================================
namespace {
inline int round_half_even(double v) { return (int)std::lrint(v); }
inline int round_half_even(float v) { return (int)std::lrintf(v); }
inline uint8_t clamp_u8(int v) { return (uint8_t)std::min(255, std::max(0, v)); }
}  // namespace

void build_gamma_lut(double k, uint8_t lut[256]) {
  for (int i = 0; i < 256; i++) {
    float f = (float)(i / 255.0);
    f = (float)std::pow((double)f, k);
    lut[i] = clamp_u8(round_half_even((double)f * 255.0));  // saturate_cast<uchar>(double)
  }
}

namespace {
// OpenCV's cubeRoot(): exponent split + quartic rational polynomial (relative error < 2^-24)
float opencv_cbrt(float value) {
  uint32_t bits;
  std::memcpy(&bits, &value, 4);
  if ((bits << 1) == 0) return 0.f;
  uint32_t sign = bits & 0x80000000u;
  int32_t mag = (int32_t)(bits & 0x7fffffffu);
  int e = (mag >> 23) - 127;
  int rem = e % 3;
  if (rem >= 0) rem -= 3;
  int e3 = (e - rem) / 3;
  uint32_t mant_bits = (uint32_t)((mag & 0x7fffff) | ((rem + 127) << 23));
  float mant;
  std::memcpy(&mant, &mant_bits, 4);
  double t = mant;  // 0.125 <= t < 1
  double num = (((45.2548339756803022511987494 * t + 192.2798368355061050458134625) * t + 119.1654824285581628956914143) * t +
                13.43250139086239872172837314) * t + 0.1636161226585754240958355063;
  double den = (((14.80884093219134573786480845 * t + 151.9714051044435648658557668) * t + 168.5254414101568283957668343) * t +
                33.9905941350215598754191872) * t + 1.0;
  float root = (float)(num / den);
  uint32_t rb;
  std::memcpy(&rb, &root, 4);
  rb = rb + ((uint32_t)e3 << 23) + sign;
  float out;
  std::memcpy(&out, &rb, 4);
  return out;
}

float srgb_to_linear(float x) {
  const float threshold = 809.f / 20000.f, low_scale = 323.f / 25.f, power = 12.f / 5.f, shift = 11.f / 200.f;
  if (x <= threshold) return x / low_scale;
  float base = (x + shift) / (1.0f + shift);
  return (float)std::pow((double)base, (double)power);
}

float linear_to_srgb(float x) {
  const float threshold = 7827.f / 2500000.f, low_scale = 323.f / 25.f, power = 12.f / 5.f, shift = 11.f / 200.f;
  if (x <= threshold) return x * low_scale;
  float inv_power = 1.0f / power;
  float p = (float)std::pow((double)x, (double)inv_power);
  return p * (1.0f + shift) - shift;
}

ColorTables make_color_tables() {
  ColorTables t;
  const int gamma_shift = 3, lab_shift = 12, lab_shift2 = lab_shift + gamma_shift, base = 1 << 14;
  const float gamma_scale = 255.f * (1 << gamma_shift);
  for (int i = 0; i < 256; i++) t.srgb_gamma[i] = (uint16_t)round_half_even(gamma_scale * srgb_to_linear((float)i / 255.f));
  for (int i = 0; i < 4096; i++) t.inv_gamma[i] = (uint16_t)round_half_even(255.f * linear_to_srgb((1.0f / 4096) * (float)i));
  {
    const float thresh = 216.f / 24389.f, slope = 841.f / 108.f, offset = 16.f / 116.f;
    const float step = 1.0f / gamma_scale;
    for (int i = 0; i < 3072; i++) {
      float x = step * (float)i;
      float f = x < thresh ? std::fmaf(x, slope, offset) : opencv_cbrt(x);
      t.cbrt[i] = (uint16_t)round_half_even((float)(1 << lab_shift2) * f);
    }
  }
  for (int i = 0; i < 256; i++) {
    int y, ify;
    if (i <= 20) {  // L <= 8: linear segment of f^-1
      y = round_half_even((float)(i * base * 20 * 9) / (float)(17 * 29 * 29 * 29));
      ify = round_half_even((float)base * (16.f / 116.f + (float)(i * 5) / (float)(3 * 17 * 29)));
    } else {
      float fy = (float)(i * 100 * base) / (float)(255 * 116) + (float)(16 * base) / 116.f;
      ify = round_half_even(fy);
      y = round_half_even(fy * fy * fy / (float)(base * base));
    }
    t.lab_to_yf[2 * i] = (uint16_t)y;
    t.lab_to_yf[2 * i + 1] = (uint16_t)ify;
  }
  const double rgb2xyz[3][3] = {{0.412453, 0.357580, 0.180423}, {0.212671, 0.715160, 0.072169}, {0.019334, 0.119193, 0.950227}};
  const double xyz2rgb[3][3] = {{3.240479, -1.53715, -0.498535}, {-0.969256, 1.875991, 0.041556}, {0.055648, -0.204043, 1.057311}};
  const double white[3] = {0.950456, 1., 1.088754};
  const double q12 = 4096.0;
  for (int row = 0; row < 3; row++)       // X, Y, Z
    for (int ch = 0; ch < 3; ch++)        // memory order B, G, R  <-  matrix column R, G, B
      t.fwd[row * 3 + ch] = round_half_even(q12 * rgb2xyz[row][2 - ch] / white[row]);
  for (int ch = 0; ch < 3; ch++)          // output rows B, G, R  <-  matrix rows R, G, B
    for (int k = 0; k < 3; k++)           // multiplies X, Y, Z
      t.inv[ch * 3 + k] = round_half_even(q12 * xyz2rgb[2 - ch][k] * white[k]);
  t.sdiv[0] = t.hdiv180[0] = 0;
  for (int i = 1; i < 256; i++) {
    t.sdiv[i] = round_half_even((255 << 12) / (1. * i));
    t.hdiv180[i] = round_half_even((180 << 12) / (6. * i));
  }
  return t;
}
}  // namespace

const ColorTables& color_tables() {
  static const ColorTables t = make_color_tables();
  return t;
}

// ---------------------------------------------------------------------------------------------
// Vignetting
// ---------------------------------------------------------------------------------------------
// vignetting_correction.cpp:32-63, operation by operation: r = sqrt(pow(dy, 2) + pow(dx, 2)) in double,
// k = pow(r, 2) * a2 + pow(r, 4) * a4, stored as float; mask = k / max (x float(1 / max)), x float(scale), + 1.0f.
// The same libm the reference would call does the work (the sqrt -> pow detour matters: with a2 = 1e-3, a4 = 1e-6
// k lands on float rounding ties often enough that the algebraically equal s * a2 + s^2 * a4 differs in ~1e-3 of
// the pixels).  k depends on (|row - rows/2|, |col - cols/2|) only, so one quadrant is evaluated and mirrored --
// the per-pixel operands are identical, only the number of pow() calls drops.  Once per (geometry, parameters);
// the reference rebuilds it on every non-square frame (quirk Q6).
// fp_contract = 1: the reference's own translation unit compiled for an FMA target (aarch64): pow(., 2) is a multiply and both
// sums of products contract -- r = sqrt(fma(dx, dx, dy * dy)), k = fma(r^2, a2, r^4 * a4) (oracle/rip_oracle.c mode 1).
void build_vignette_mask(int rows, int cols, double scale, double a2, double a4, std::vector<float>& mask, int fp_contract) {
  mask.resize((size_t)rows * cols);
  const double cy = rows / 2.0, cx = cols / 2.0;
  // distinct |2 * d| values per axis: index = |2 * i - n|
  std::vector<float> quad((size_t)(rows + 1) * (cols + 1), 0.f);
  std::vector<char> have((size_t)(rows + 1) * (cols + 1), 0);
  float mx = -FLT_MAX;
  for (int row = 0; row < rows; row++) {
    const int ay = std::abs(2 * row - rows);
    for (int col = 0; col < cols; col++) {
      const int ax = std::abs(2 * col - cols);
      const size_t qi = (size_t)ay * (cols + 1) + ax;
      if (!have[qi]) {
        const double dy = std::fabs(row - cy), dx = std::fabs(col - cx);
        double r = std::sqrt(std::pow(dx, 2) + std::pow(dy, 2));
        double k = std::pow(r, 2) * a2 + std::pow(r, 4) * a4;
        if (fp_contract) {
          r = std::sqrt(std::fma(dx, dx, dy * dy));
          k = std::fma(std::pow(r, 2), a2, std::pow(r, 4) * a4);
        }
        quad[qi] = (float)k;
        have[qi] = 1;
      }
      const float kf = quad[qi];
      mask[(size_t)row * cols + col] = kf;
      if (kf > mx) mx = kf;
    }
  }
  const double maxv = (double)mx;
  const size_t n = mask.size();
  if (maxv > 0) {
    const float inv = (float)(1.0 / maxv);
    for (size_t i = 0; i < n; i++) mask[i] = mask[i] * inv;
  }
  const float sc = (float)scale;
  for (size_t i = 0; i < n; i++) mask[i] = mask[i] * sc;
  for (size_t i = 0; i < n; i++) mask[i] = mask[i] + 1.0f;
}

}  // namespace rip
