// csrc/rip_yaml.cpp, rip_params.cpp and rip_output_tables.cpp on their own: no HIP header, no HIP library, nothing else of
// librip_hip.so -- that this program links is the proof that the three units stand without the rest.  It loads a parameter text with
// an `output:` and an `output_2:` section and checks fields of the result; gives every check function of a setting one refused
// value, directly (std::invalid_argument) and through a parameter text (the load throws the same and leaves Modules as it was); and
// compares output_window_geometry for one letterbox and one crop case with numbers worked out by hand.  Stand-alone: may be built
// with -fsanitize=address,undefined.
// usage: host_units_test <scratch file>
#include <cstdio>
#include <fstream>
#include <functional>
#include <sstream>
#include <string>

#include "rip_output_tables.hpp"
#include "rip_params.hpp"
#include "rip_yaml.hpp"

static int g_checks = 0, g_bad = 0;

static void check(bool ok, const std::string& what) {
  g_checks++;
  if (!ok && g_bad++ < 20) std::printf("bad: %s\n", what.c_str());
}

// every field of Modules, in text
static std::string dump(const rip::Modules& m) {
  std::ostringstream s;
  s.precision(17);
  s << m.use_gpu << m.debug << m.debayer_enabled << ' ' << m.debayer_encoding << ' ' << m.debayer_16bit << ' ' << m.raw16_black << ' ' << m.raw16_white << ' '
    << m.debayer_method << ' ' << m.n_heads << ' ' << m.selected << '\n';
  for (const rip::OutputHead& h : m.heads) {
    s << h.out_format << ' ' << h.out_yuv_matrix << ' ' << h.out_divisor << ' ' << h.out_w << ' ' << h.out_h << ' ' << h.out_interp << ' ' << h.roi_x << ' '
      << h.roi_y << ' ' << h.roi_w << ' ' << h.roi_h << ' ' << h.out_fit;
    for (int i = 0; i < 3; i++) s << ' ' << h.out_mean[i] << ' ' << h.out_std[i] << ' ' << h.out_pad[i];
    s << '\n';
  }
  s << m.flip_enabled << ' ' << m.flip_angle << ' ' << m.wb_enabled << ' ' << m.wb_method << ' ' << m.wb_percentile << ' ' << m.wb_bright_thr << ' '
    << m.wb_dark_thr << ' ' << m.wb_temporal << ' ' << m.cc_enabled << ' ' << m.cc_available << ' ' << m.gamma_enabled << ' ' << m.gamma_method << ' '
    << m.gamma_k << ' ' << m.vig_enabled << ' ' << m.vig_scale << ' ' << m.vig_a2 << ' ' << m.vig_a4 << ' ' << m.ce_enabled << ' ' << m.ce_value_gain << ' '
    << m.ce_saturation_gain << ' ' << m.ce_hue_gain << ' ' << m.und_enabled << ' ' << m.und_available << ' ' << m.dist_model << ' ' << m.rect_model << ' '
    << m.dist_w << ' ' << m.dist_h << ' ' << m.rect_w << ' ' << m.rect_h << ' ' << m.balance << ' ' << m.fov_scale << ' ' << m.rect_mask << '\n';
  for (int i = 0; i < 9; i++) s << m.cc_matrix[i] << ' ' << m.dist_K[i] << ' ' << m.rect_K[i] << ' ' << m.dist_R[i] << ' ' << m.rect_R[i] << ' ';
  for (int i = 0; i < 4; i++) s << m.cc_bias[i] << ' ';
  for (int i = 0; i < 8; i++) s << m.dist_D[i] << ' ' << m.rect_D[i] << ' ';
  for (int i = 0; i < 12; i++) s << m.dist_P[i] << ' ' << m.rect_P[i] << ' ';
  return s.str();
}

static bool load_text(rip::Modules& m, const std::string& path, const std::string& text) {
  std::ofstream(path) << text;
  return rip::load_params_file(m, path);
}

static bool refuses(const std::function<void()>& call) {
  try {
    call();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: host_units_test <scratch file>\n");
    return 2;
  }
  const std::string path = argv[1];
  rip::Modules m;

  // 1, 2: two sections of output settings, a gap between them
  const std::string text =
      "flip:\n  enabled: true\n  angle: 180\n"
      "undistortion:\n  enabled: true\n  mask: valid   # a comment\n"
      "output:\n  format: rgb8\n  size: [40, 20]\n  fit: letterbox\n  pad: [1, 2, 3]\n"
      "output_2:\n  format: bgr_chw_f16\n  divisor: 1.0\n  mean: [0.5, 0.25, 0.125]\n  std: [2.0, 0.5, 1.5]\n  roi: [8, 4, 32, 24]\n"
      "  interpolation: cubic_aa\n  yuv_matrix: bt709_full\n";
  check(load_text(m, path, text), "the load of an existing file returns true");
  check(m.n_heads == 3 && m.selected == 0, "output_2: makes three heads, head 0 selected");
  check(m.flip_enabled && m.flip_angle == 180 && m.und_enabled && m.rect_mask == "valid", "flip and undistortion sections");
  check(m.gamma_k == 0.8 && m.wb_method == "ccc" && !m.wb_enabled, "absent sections hold the loader's defaults");
  const rip::OutputHead &h0 = m.heads[0], &h1 = m.heads[1], &h2 = m.heads[2];
  check(h0.out_format == "rgb8" && h0.out_w == 40 && h0.out_h == 20 && h0.out_fit == "letterbox", "output: format, size, fit");
  check(h0.out_pad[0] == 1 && h0.out_pad[1] == 2 && h0.out_pad[2] == 3 && h0.out_interp == "linear" && h0.roi_w == 0, "output: pad, and defaults of the absent keys");
  check(h1.out_format == "native" && h1.out_w == 0 && h1.out_fit == "stretch" && h1.out_pad[0] == 114, "the section in between holds the defaults");
  check(h2.out_format == "bgr_chw_f16" && h2.out_divisor == 1.0 && h2.out_mean[1] == 0.25 && h2.out_std[2] == 1.5, "output_2: format and normalisation");
  check(h2.roi_x == 8 && h2.roi_y == 4 && h2.roi_w == 32 && h2.roi_h == 24 && h2.out_interp == "cubic_aa" && h2.out_yuv_matrix == "bt709_full",
        "output_2: roi, interpolation, yuv_matrix");
  check(!rip::load_params_file(m, path + ".absent"), "a missing file is a soft failure");
  check(rip::output_format_id("bgr_chw_f16") == 7 && rip::output_fit_id("crop") == 2 && rip::output_interpolation_id("cubic_aa") == 3 &&
            rip::output_yuv_matrix_id("bt709_full") == 3 && rip::rect_mask_mode_id("valid") == 2,
        "the ids of accepted names");

  // 3: one refused value per check function, directly and through a text that would otherwise turn the flip off
  const double zero3[3] = {0, 0, 0}, one3[3] = {1, 1, 1};
  const struct {
    const char* name;
    std::function<void()> call;
    const char* section;
  } refused[] = {
      {"rect_mask_mode_id", [] { (void)rip::rect_mask_mode_id("sometimes"); }, "undistortion:\n  mask: sometimes\n"},
      {"check_debayer_method", [] { rip::check_debayer_method("nearest"); }, "debayer:\n  method: nearest\n"},
      {"check_debayer_16bit_range", [] { rip::check_debayer_16bit_range(9, 3); }, "debayer:\n  black_level: 9\n  white_level: 3\n"},
      {"output_format_id", [] { (void)rip::output_format_id("nope"); }, "output:\n  format: nope\n"},
      {"output_yuv_matrix_id", [] { (void)rip::output_yuv_matrix_id("bt2020"); }, "output:\n  yuv_matrix: bt2020\n"},
      {"output_interpolation_id", [] { (void)rip::output_interpolation_id("nearest"); }, "output_2:\n  interpolation: nearest\n"},
      {"output_fit_id", [] { (void)rip::output_fit_id("fill"); }, "output:\n  fit: fill\n"},
      {"check_output_normalization", [&] { rip::check_output_normalization(0.0, zero3, one3); }, "output:\n  divisor: 0\n"},
      {"check_output_size", [] { rip::check_output_size(0, 5); }, "output_1:\n  size: [0, 5]\n"},
      {"check_output_roi", [] { rip::check_output_roi(1, 1, 0, 4); }, "output:\n  roi: [1, 1, 0, 4]\n"},
      {"check_output_pad", [] { rip::check_output_pad(1, 2, 300); }, "output:\n  pad: [1, 2, 300]\n"},
  };
  const std::string before = dump(m);
  for (const auto& r : refused) {
    check(refuses(r.call), std::string(r.name) + " throws std::invalid_argument");
    check(refuses([&] { load_text(m, path, std::string("flip:\n  enabled: false\n") + r.section); }), std::string(r.name) + ": the load throws std::invalid_argument");
    check(dump(m) == before, std::string(r.name) + ": the refused load leaves Modules as it was");
  }
  check(load_text(m, path, "flip:\n  enabled: false\n") && dump(m) != before && !m.flip_enabled && m.n_heads == 1, "the same text without a refused value loads");

  // 4: a 64 x 48 image into 40 x 20.  Letterbox: the scale is min(40 / 64, 20 / 48) = 5 / 12, so the picture is 20 rows high and
  // 64 * 5 / 12 = 26.67 -> 27 columns wide, centred: (40 - 27) / 2 = 6 columns of pad on the left.  Crop of the window (8, 4, 32, 24): the
  // target is twice as wide as high, so of the 32 columns' 24 rows 16 are read, centred: 4 + (24 - 16) / 2 = 8.
  int src[4], dst[4];
  const int all[4] = {0, 0, 0, 0}, window[4] = {8, 4, 32, 24};
  rip::output_window_geometry(64, 48, all, 40, 20, rip::output_fit_id("letterbox"), src, dst);
  check(src[0] == 0 && src[1] == 0 && src[2] == 64 && src[3] == 48 && dst[0] == 6 && dst[1] == 0 && dst[2] == 27 && dst[3] == 20, "letterbox geometry");
  rip::output_window_geometry(64, 48, window, 40, 20, rip::output_fit_id("crop"), src, dst);
  check(src[0] == 8 && src[1] == 8 && src[2] == 32 && src[3] == 16 && dst[0] == 0 && dst[1] == 0 && dst[2] == 40 && dst[3] == 20, "crop geometry");
  check(refuses([&] { rip::output_window_geometry(64, 48, window, 0, 0, 0, src, dst); }) == false && src[2] == 32 && dst[2] == 32, "a window without a target is delivered as it is");
  const int outside[4] = {40, 4, 32, 24};
  check(refuses([&] { rip::output_window_geometry(64, 48, outside, 0, 0, 0, src, dst); }), "a window outside the image is refused");

  std::remove(path.c_str());
  std::printf("%d checks, %d bad\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
