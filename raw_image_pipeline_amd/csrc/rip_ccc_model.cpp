// rip_ccc_model.cpp -- ccc model, host FFT and scalar tables (rip_ccc_model.hpp).
// Float expressions here define bit patterns the kernels depend on: compile with -ffp-contract=off (build.py does).
#include "rip_ccc_model.hpp"

#include <cmath>
#include <cstdint>
#include <fstream>
#include <stdexcept>

namespace rip {

// ---------------------------------------------------------------------------------------------
// CCC model
// ---------------------------------------------------------------------------------------------
void fft256_twiddles(float re[128], float im[128]) {
  for (int k = 0; k < 128; k++) {
    double ang = -2.0 * 3.14159265358979323846 * k / 256;
    re[k] = (float)std::cos(ang);
    im[k] = (float)std::sin(ang);
  }
}

namespace {
// Reference 256-point radix-2 DIT FFT on interleaved complex data with element stride (in
// complex elements).  Butterfly order and arithmetic are the contract the kernels follow.
void host_fft256(float* data, int stride, const float* twr, const float* twi, bool inverse) {
  float buf[512];
  for (int i = 0; i < 256; i++) {
    unsigned r = (unsigned)i;
    r = ((r & 0xF0u) >> 4) | ((r & 0x0Fu) << 4);
    r = ((r & 0xCCu) >> 2) | ((r & 0x33u) << 2);
    r = ((r & 0xAAu) >> 1) | ((r & 0x55u) << 1);
    buf[2 * r] = data[2 * (size_t)i * stride];
    buf[2 * r + 1] = data[2 * (size_t)i * stride + 1];
  }
  for (int len = 2; len <= 256; len <<= 1) {
    int half = len / 2, tstep = 256 / len;
    for (int b = 0; b < 128; b++) {
      int k = b % half, lo = (b / half) * len + k, hi = lo + half;
      float wr = twr[k * tstep], wi = inverse ? -twi[k * tstep] : twi[k * tstep];
      float xr = buf[2 * hi], xi = buf[2 * hi + 1];
      float tr = wr * xr - wi * xi;
      float ti = wr * xi + wi * xr;
      float ur = buf[2 * lo], ui = buf[2 * lo + 1];
      buf[2 * lo] = ur + tr;
      buf[2 * lo + 1] = ui + ti;
      buf[2 * hi] = ur - tr;
      buf[2 * hi + 1] = ui - ti;
    }
  }
  for (int i = 0; i < 256; i++) {
    data[2 * (size_t)i * stride] = buf[2 * i];
    data[2 * (size_t)i * stride + 1] = buf[2 * i + 1];
  }
}

void host_fft2d(std::vector<float>& c, const float* twr, const float* twi) {
  for (int r = 0; r < 256; r++) host_fft256(c.data() + 2 * (size_t)r * 256, 1, twr, twi, false);
  for (int col = 0; col < 256; col++) host_fft256(c.data() + 2 * (size_t)col, 256, twr, twi, false);
}
}  // namespace

void ccc_build_model(CccModel& m, int w, int h, const float* filter, const float* bias) {
  if (w != 256 || h != 256) throw std::invalid_argument("CCC model must be 256x256 (got " + std::to_string(w) + "x" + std::to_string(h) + ")");
  float twr[128], twi[128];
  fft256_twiddles(twr, twi);
  m.filter_t.assign(65536, 0.f);
  m.bias_t.assign(65536, 0.f);
  m.filter_fft.assign(131072, 0.f);
  m.bias_fft.assign(131072, 0.f);
  for (int y = 0; y < 256; y++)
    for (int x = 0; x < 256; x++) {
      // loadModel transposes both planes (convolutional_color_constancy.cpp:131-132)
      float f = filter[(size_t)x * 256 + y], b = bias[(size_t)x * 256 + y];
      m.filter_t[(size_t)y * 256 + x] = f;
      m.bias_t[(size_t)y * 256 + x] = b;
      m.filter_fft[2 * ((size_t)y * 256 + x)] = f;
      m.bias_fft[2 * ((size_t)y * 256 + x)] = b;
    }
  host_fft2d(m.filter_fft, twr, twi);
  host_fft2d(m.bias_fft, twr, twi);
  m.loaded = true;
}

bool ccc_load_model_file(CccModel& m, const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f.good()) return false;
  int32_t w = 0, h = 0;
  f.read((char*)&w, 4);
  f.read((char*)&h, 4);
  if (!f.good() || w <= 0 || h <= 0 || (int64_t)w * h > (1 << 20)) throw std::invalid_argument("CCC model file " + path + ": bad header");
  std::vector<float> filt((size_t)w * h), bias((size_t)w * h);
  f.read((char*)filt.data(), (std::streamsize)filt.size() * 4);
  f.read((char*)bias.data(), (std::streamsize)bias.size() * 4);
  if (!f.good()) throw std::invalid_argument("CCC model file " + path + ": truncated");
  ccc_build_model(m, w, h, filt.data(), bias.data());
  return true;
}

void ccc_build_scalar_tables(float log_tab[256], std::vector<float>& accum_tab, float exp_neg_tab[256]) {
  log_tab[0] = -INFINITY;
  for (int i = 1; i < 256; i++) log_tab[i] = std::log((float)i);
  const int n = 360 * 270;
  float num_pixels = (float)n;
  float weight = 1.0f / num_pixels;
  accum_tab.assign(n + 1, 0.f);
  float acc = 0.f;
  for (int i = 1; i <= n; i++) {
    acc += weight;
    accum_tab[i] = acc;
  }
  const float bin = 1.0f / 64.0f, uv0 = -1.421875f;
  for (int k = 0; k < 256; k++) {
    float L = k * bin + uv0;
    exp_neg_tab[k] = std::exp(-L);
  }
}

}  // namespace rip
