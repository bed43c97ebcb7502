// rip_ccc_model.hpp -- the ccc estimator's model on the host: the spectra of filter and bias, the FFT they are built with and the
// scalar tables of the device-side estimator.
#pragma once
#include <string>
#include <vector>

namespace rip {

// ---------------------------------------------------------------------------------------------
// CCC model (convolutional_color_constancy.cpp:116-207)
// ---------------------------------------------------------------------------------------------
struct CccModel {
  bool loaded = false;
  std::vector<float> filter_fft;  // 256*256 complex (re,im interleaved), FFT of the transposed filter
  std::vector<float> bias_fft;    // idem for the bias
  std::vector<float> filter_t, bias_t;  // transposed spatial copies (tests)
};
void ccc_build_model(CccModel& m, int w, int h, const float* filter, const float* bias);  // throws std::invalid_argument
bool ccc_load_model_file(CccModel& m, const std::string& path);                           // false: unreadable
// 128 complex twiddles of the radix-2 256-point FFT (shared with the kernels)
void fft256_twiddles(float re[128], float im[128]);
// Tables used by the device-side ccc estimator so that its float results do not depend on
// device transcendental implementations: ln(i) for i in 0..255 (ln 0 = -inf), the value of
// a histogram bin after n sequential float additions of 1/97200, and exp(-(k/64 + uv0)).
void ccc_build_scalar_tables(float log_tab[256], std::vector<float>& accum_tab, float exp_neg_tab[256]);

}  // namespace rip
