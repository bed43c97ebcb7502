// rip_settings.cpp -- the settings half of the C ABI (include/rip.h): the loaders, the output heads, every setter and every getter
// of a module parameter, and the tunables.  A setter checks, assigns, and names what it invalidates through the helpers of
// rip_constants.cpp (invalidate_*, und_init); no flag of a cached constant is written here.  The order of the statements inside a
// setter is part of its behaviour: what runs before a refusal stays done (tests/test_setter_effects_gpu.py).
#include <cstring>

#include "rip_handle.hpp"

using namespace rip::api;

namespace {
// the getters of a string and of a vector of doubles
template <typename Value>
rip_status get_string(const rip_pipeline* p, char* out, size_t cap, Value&& value) {
  return guarded(p, [&] {
    need(p);
    copy_string(value(), out, cap);
  });
}
template <typename T>
rip_status get_vec(const rip_pipeline* p, double* out, const T* field, int n) {
  return guarded(p, [&] {
    need(p);
    if (!out) throw InvalidArgument("null output");
    for (int i = 0; i < n; i++) out[i] = (double)field[i];
  });
}
}  // namespace

#pragma GCC visibility push(default)
extern "C" {

// ---- output heads --------------------------------------------------------------------------------
rip_status rip_set_output_heads(rip_pipeline* p, int n) {
  return guarded(p, [&] {
    need(p);
    if (n < 1 || n > RIP_MAX_OUTPUT_HEADS) throw InvalidArgument("output heads: 1.." + std::to_string(RIP_MAX_OUTPUT_HEADS) + " expected, got " + std::to_string(n));
    for (auto& s : p->ring)
      if (s->busy) throw InvalidArgument("rip_set_output_heads: frames are in flight");
    for (int k = n; k < RIP_MAX_OUTPUT_HEADS; k++) {
      p->m.heads[k] = rip::OutputHead();
      p->head_record[k] = {};
      p->jpeg_frames[k] = 0;
      invalidate_head(p, k, true);
    }
    p->m.n_heads = n;
    if (p->m.selected >= n) p->m.selected = 0;
  });
}
rip_status rip_get_output_heads(rip_pipeline* p, int* n) {
  return guarded(p, [&] {
    need(p);
    if (n) *n = p->m.n_heads;
  });
}
rip_status rip_select_output_head(rip_pipeline* p, int head) {
  return guarded(p, [&] {
    need(p);
    need_head(p, head);
    p->m.selected = head;
  });
}
rip_status rip_get_selected_output_head(rip_pipeline* p, int* head) {
  return guarded(p, [&] {
    need(p);
    if (head) *head = p->m.selected;
  });
}

// ---- valid-pixel masks ---------------------------------------------------------------------------
rip_status rip_set_rect_mask(rip_pipeline* p, const char* mode) {
  return guarded(p, [&] {
    need(p);
    if (!mode) throw InvalidArgument("null string");
    (void)rip::rect_mask_mode_id(mode);
    p->m.rect_mask = mode;
  });
}
rip_status rip_get_rect_mask_mode(const rip_pipeline* p, char* out, size_t capacity) {
  return get_string(p, out, capacity, [&] { return p->m.rect_mask; });
}

// ---- loaders -----------------------------------------------------------------------------------
rip_status rip_load_params(rip_pipeline* p, const char* path) {
  return guarded(p, [&] {
    need(p);
    if (!path) throw InvalidArgument("path is null");
    std::fprintf(stderr, "Loading raw_image_pipeline params from file %s\n", path);
    if (!rip::load_params_file(p->m, path)) {
      std::fprintf(stderr, "Warning: parameters file doesn't exist\n");  // nothing else happens (:162-164)
    } else {
      // loadParams re-creates every module (std::make_unique, raw_image_pipeline.cpp:56-160): whatever
      // loadColorCalibration / loadCameraCalibration had loaded is gone (identity matrix, calibration not available --
      // the constructors reload them afterwards, :27-29), and the white balancer starts over with a fresh ccc
      // estimator (first frame, new Kalman filter)
      const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
      for (int i = 0; i < 9; i++) p->m.cc_matrix[i] = (float)eye[i];
      for (int i = 0; i < 4; i++) p->m.cc_bias[i] = 0;
      p->m.cc_available = false;
      p->m.und_available = false;
      restart_ccc_estimator(p);
    }
    invalidate_color_tables(p);
    invalidate_vignette(p);
    invalidate_ccc_config(p);
    invalidate_all_heads(p);
    und_init(p);  // setBalance / setFovScale re-run init()
  });
}
rip_status rip_load_camera_calibration(rip_pipeline* p, const char* path) {
  return guarded(p, [&] {
    need(p);
    if (!path) throw InvalidArgument("path is null");
    std::fprintf(stderr, "Loading camera calibration from file %s\n", path);
    if (!rip::load_camera_calibration_file(p->m, path)) std::fprintf(stderr, "Warning: Calibration file doesn't exist\n");
    und_init(p);
  });
}
rip_status rip_load_color_calibration(rip_pipeline* p, const char* path) {
  return guarded(p, [&] {
    need(p);
    if (!path) throw InvalidArgument("path is null");
    std::fprintf(stderr, "Loading color calibration from file %s\n", path);
    if (!rip::load_color_calibration_file(p->m, path)) std::fprintf(stderr, "Warning: Color calibration file doesn't exist\n");
  });
}
rip_status rip_load_ccc_model(rip_pipeline* p, const char* path) {
  return guarded(p, [&] {
    need(p);
    if (!path) throw InvalidArgument("path is null");
    if (!rip::ccc_load_model_file(p->ccc.model, path)) throw rip::YamlError(std::string("cannot read CCC model ") + path);
    invalidate_ccc_model(p);
  });
}
rip_status rip_set_ccc_model(rip_pipeline* p, int w, int h, const float* filter, const float* bias) {
  return guarded(p, [&] {
    need(p);
    if (!filter || !bias) throw InvalidArgument("null model planes");
    rip::ccc_build_model(p->ccc.model, w, h, filter, bias);
    invalidate_ccc_model(p);
  });
}

// ---- setters -----------------------------------------------------------------------------------
rip_status rip_set_taps(rip_pipeline* p, int mask) {
  return guarded(p, [&] {
    need(p);
    p->tap_mask = mask & 7;
  });
}
rip_status rip_set_tap_download(rip_pipeline* p, int mask) {
  return guarded(p, [&] {
    need(p);
    p->tap_download_mask = mask & (RIP_TAP_DEBAYERED | RIP_TAP_COLOR);
  });
}
rip_status rip_set_ccc_kalman_model(rip_pipeline* p, double h, double r) {
  return guarded(p, [&] {
    need(p);
    p->ccc.kf_h = h;
    p->ccc.kf_r = r;
    invalidate_ccc_config(p);
  });
}
rip_status rip_reset_white_balance_temporal_consistency(rip_pipeline* p) {
  return guarded(p, [&] {
    need(p);
    if (p->m.wb_method == "ccc") p->ccc.reset_pending = true;  // white_balance.cpp:42-47
  });
}
rip_status rip_set_gpu(rip_pipeline* p, int v) {
  return guarded(p, [&] {
    need(p);
    p->m.use_gpu = v != 0;
  });
}
rip_status rip_set_debug(rip_pipeline* p, int v) {
  return guarded(p, [&] {
    need(p);
    p->m.debug = v != 0;
  });
}
rip_status rip_set_debayer(rip_pipeline* p, int v) {
  return guarded(p, [&] {
    need(p);
    p->m.debayer_enabled = v != 0;
  });
}
rip_status rip_set_debayer_16bit(rip_pipeline* p, int v) {
  return guarded(p, [&] {
    need(p);
    p->m.debayer_16bit = v != 0;
  });
}
rip_status rip_set_debayer_16bit_range(rip_pipeline* p, int black, int white) {
  return guarded(p, [&] {
    need(p);
    rip::check_debayer_16bit_range(black, white);
    p->m.raw16_black = black;
    p->m.raw16_white = white;
  });
}
rip_status rip_set_debayer_encoding(rip_pipeline* p, const char* s) {
  return guarded(p, [&] {
    need(p);
    if (!s) throw InvalidArgument("null string");
    p->m.debayer_encoding = s;
  });
}
rip_status rip_set_debayer_method(rip_pipeline* p, const char* s) {
  return guarded(p, [&] {
    need(p);
    if (!s) throw InvalidArgument("null string");
    rip::check_debayer_method(s);
    p->m.debayer_method = s;
  });
}
// An output setter of the selected head drops that head's delivered mask (rip_get_output_mask) first, whatever it sets and whether
// or not the value is then refused; rip_set_output_yuv_matrix, which no mask depends on, is the exception.
rip_status rip_set_output_format(rip_pipeline* p, const char* s) {
  return guarded(p, [&] {
    need(p);
    invalidate_head(p, p->m.selected, false);
    if (!s) throw InvalidArgument("null string");
    (void)rip::output_format_id(s);
    if (p->m.out().out_format != s) invalidate_head(p, p->m.selected, true);
    p->m.out().out_format = s;
  });
}
rip_status rip_set_output_yuv_matrix(rip_pipeline* p, const char* s) {
  return guarded(p, [&] {
    need(p);
    if (!s) throw InvalidArgument("null string");
    (void)rip::output_yuv_matrix_id(s);
    p->m.out().out_yuv_matrix = s;
  });
}
rip_status rip_set_output_normalization(rip_pipeline* p, double divisor, const double* mean, const double* sd) {
  return guarded(p, [&] {
    need(p);
    invalidate_head(p, p->m.selected, false);
    if (!mean || !sd) throw InvalidArgument("null mean or std");
    rip::check_output_normalization(divisor, mean, sd);
    p->m.out().out_divisor = divisor;
    for (int i = 0; i < 3; i++) {
      p->m.out().out_mean[i] = mean[i];
      p->m.out().out_std[i] = sd[i];
    }
    invalidate_head(p, p->m.selected, true);
  });
}
rip_status rip_set_output_size(rip_pipeline* p, int width, int height) {
  return guarded(p, [&] {
    need(p);
    invalidate_head(p, p->m.selected, false);
    rip::check_output_size(width, height);
    p->m.out().out_w = width;
    p->m.out().out_h = height;
  });
}
rip_status rip_set_output_interpolation(rip_pipeline* p, const char* s) {
  return guarded(p, [&] {
    need(p);
    invalidate_head(p, p->m.selected, false);
    if (!s) throw InvalidArgument("null string");
    (void)rip::output_interpolation_id(s);
    p->m.out().out_interp = s;
  });
}
rip_status rip_set_output_roi(rip_pipeline* p, int x, int y, int width, int height) {
  return guarded(p, [&] {
    need(p);
    invalidate_head(p, p->m.selected, false);
    rip::check_output_roi(x, y, width, height);
    p->m.out().roi_x = x;
    p->m.out().roi_y = y;
    p->m.out().roi_w = width;
    p->m.out().roi_h = height;
  });
}
rip_status rip_set_output_fit(rip_pipeline* p, const char* s) {
  return guarded(p, [&] {
    need(p);
    invalidate_head(p, p->m.selected, false);
    if (!s) throw InvalidArgument("null string");
    (void)rip::output_fit_id(s);
    p->m.out().out_fit = s;
  });
}
rip_status rip_set_output_pad(rip_pipeline* p, int b, int g, int r) {
  return guarded(p, [&] {
    need(p);
    invalidate_head(p, p->m.selected, false);
    rip::check_output_pad(b, g, r);
    p->m.out().out_pad[0] = b;
    p->m.out().out_pad[1] = g;
    p->m.out().out_pad[2] = r;
  });
}
rip_status rip_set_output_clahe(rip_pipeline* p, double clip_limit, int tiles_x, int tiles_y) {
  return guarded(p, [&] {
    need(p);
    invalidate_head(p, p->m.selected, false);
    rip::check_output_clahe(clip_limit, tiles_x, tiles_y);
    p->m.out().clahe_clip_limit = clip_limit;
    p->m.out().clahe_tiles_x = tiles_x;
    p->m.out().clahe_tiles_y = tiles_y;
  });
}
rip_status rip_set_output_jpeg(rip_pipeline* p, int quality, int restart_rows) {
  return guarded(p, [&] {
    need(p);
    invalidate_head(p, p->m.selected, false);
    rip::check_output_jpeg(quality, restart_rows);
    p->m.out().jpeg_quality = quality;
    p->m.out().jpeg_restart_rows = restart_rows;
  });
}
rip_status rip_set_flip(rip_pipeline* p, int v) {
  return guarded(p, [&] {
    need(p);
    p->m.flip_enabled = v != 0;
  });
}
rip_status rip_set_flip_angle(rip_pipeline* p, int a) {
  return guarded(p, [&] {
    need(p);
    p->m.flip_angle = a;
  });
}
rip_status rip_set_white_balance(rip_pipeline* p, int v) {
  return guarded(p, [&] {
    need(p);
    p->m.wb_enabled = v != 0;
  });
}
rip_status rip_set_white_balance_method(rip_pipeline* p, const char* s) {
  return guarded(p, [&] {
    need(p);
    if (!s) throw InvalidArgument("null string");
    p->m.wb_method = s;
  });
}
rip_status rip_set_white_balance_percentile(rip_pipeline* p, double v) {
  return guarded(p, [&] {
    need(p);
    p->m.wb_percentile = v;
  });
}
rip_status rip_set_white_balance_saturation_threshold(rip_pipeline* p, double b, double d) {
  return guarded(p, [&] {
    need(p);
    p->m.wb_bright_thr = b;
    p->m.wb_dark_thr = d;
  });
}
rip_status rip_set_white_balance_temporal_consistency(rip_pipeline* p, int v) {
  return guarded(p, [&] {
    need(p);
    p->m.wb_temporal = v != 0;
    invalidate_ccc_config(p);
  });
}
rip_status rip_set_color_calibration(rip_pipeline* p, int v) {
  return guarded(p, [&] {
    need(p);
    p->m.cc_enabled = v != 0;
  });
}
rip_status rip_set_color_calibration_matrix(rip_pipeline* p, const double* v, int n) {
  return guarded(p, [&] {
    need(p);
    if (!v || n != 9) throw InvalidArgument("color calibration matrix needs 9 values");
    for (int i = 0; i < 9; i++) p->m.cc_matrix[i] = (float)v[i];  // Matx33d -> Matx33f, color_calibration.cpp:79
  });
}
rip_status rip_set_color_calibration_bias(rip_pipeline* p, const double* v, int n) {
  return guarded(p, [&] {
    need(p);
    if (!v || n < 3) throw InvalidArgument("color calibration bias needs 3 values");  // vector::at throws
    for (int i = 0; i < 3; i++) p->m.cc_bias[i] = v[i];
    p->m.cc_bias[3] = 0;
  });
}
rip_status rip_set_gamma_correction(rip_pipeline* p, int v) {
  return guarded(p, [&] {
    need(p);
    p->m.gamma_enabled = v != 0;
    invalidate_color_tables(p);
  });
}
rip_status rip_set_gamma_correction_method(rip_pipeline* p, const char* s) {
  return guarded(p, [&] {
    need(p);
    if (!s) throw InvalidArgument("null string");
    p->m.gamma_method = s;
  });
}
rip_status rip_set_gamma_correction_k(rip_pipeline* p, double k) {
  return guarded(p, [&] {
    need(p);
    p->m.gamma_k = k;
    invalidate_color_tables(p);
  });
}
rip_status rip_set_fp_contraction(rip_pipeline* p, int mode) {
  return guarded(p, [&] {
    need(p);
    if (mode != 0 && mode != 1) throw InvalidArgument("fp contraction model must be 0 (none) or 1 (fused)");
    if (mode != p->fp_contract) invalidate_vignette(p);  // the mask plane's k = r^2 a2 + r^4 a4 is one of the contracted expressions
    p->fp_contract = mode;
  });
}
rip_status rip_set_vignetting_correction(rip_pipeline* p, int v) {
  return guarded(p, [&] {
    need(p);
    p->m.vig_enabled = v != 0;
  });
}
rip_status rip_set_vignetting_correction_parameters(rip_pipeline* p, double s, double a2, double a4) {
  return guarded(p, [&] {
    need(p);
    p->m.vig_scale = s;
    p->m.vig_a2 = a2;
    p->m.vig_a4 = a4;
    invalidate_vignette(p);
  });
}
rip_status rip_set_color_enhancer(rip_pipeline* p, int v) {
  return guarded(p, [&] {
    need(p);
    p->m.ce_enabled = v != 0;
  });
}
// cross-wired exactly as color_enhancer.cpp:23-33
rip_status rip_set_color_enhancer_hue_gain(rip_pipeline* p, double g) {
  return guarded(p, [&] {
    need(p);
    p->m.ce_value_gain = g;
  });
}
rip_status rip_set_color_enhancer_saturation_gain(rip_pipeline* p, double g) {
  return guarded(p, [&] {
    need(p);
    p->m.ce_saturation_gain = g;
  });
}
rip_status rip_set_color_enhancer_value_gain(rip_pipeline* p, double g) {
  return guarded(p, [&] {
    need(p);
    p->m.ce_hue_gain = g;
  });
}
rip_status rip_set_undistortion(rip_pipeline* p, int v) {
  return guarded(p, [&] {
    need(p);
    p->m.und_enabled = v != 0;
  });
}
rip_status rip_set_undistortion_image_size(rip_pipeline* p, int w, int h) {
  return guarded(p, [&] {
    need(p);
    p->m.dist_w = p->m.rect_w = w;
    p->m.dist_h = p->m.rect_h = h;
    und_init(p);
  });
}
rip_status rip_set_undistortion_new_image_size(rip_pipeline* p, int w, int h) {
  return guarded(p, [&] {
    need(p);
    p->m.rect_w = w;
    p->m.rect_h = h;
    und_init(p);
  });
}
rip_status rip_set_undistortion_balance(rip_pipeline* p, double b) {
  return guarded(p, [&] {
    need(p);
    p->m.balance = b;
    und_init(p);
  });
}
rip_status rip_set_undistortion_fov_scale(rip_pipeline* p, double f) {
  return guarded(p, [&] {
    need(p);
    p->m.fov_scale = f;
    und_init(p);
  });
}
rip_status rip_set_undistortion_camera_matrix(rip_pipeline* p, const double* v, int n) {
  return guarded(p, [&] {
    need(p);
    if (!v || n < 9) throw InvalidArgument("camera matrix needs 9 values");
    for (int i = 0; i < 9; i++) p->m.dist_K[i] = p->m.rect_K[i] = v[i];
    und_init(p);
  });
}
rip_status rip_set_undistortion_distortion_coefficients(rip_pipeline* p, const double* v, int n) {
  return guarded(p, [&] {
    need(p);
    if (!v || n < 4) throw InvalidArgument("distortion coefficients need 4 values");
    for (int i = 0; i < 8; i++) p->m.dist_D[i] = p->m.rect_D[i] = i < n ? v[i] : 0.0;
    und_init(p);
  });
}
rip_status rip_set_undistortion_distortion_model(rip_pipeline* p, const char* s) {
  return guarded(p, [&] {
    need(p);
    if (!s) throw InvalidArgument("null string");
    p->m.dist_model = p->m.rect_model = s;
    und_init(p);
  });
}
rip_status rip_set_undistortion_rectification_matrix(rip_pipeline* p, const double* v, int n) {
  return guarded(p, [&] {
    need(p);
    if (!v || n < 9) throw InvalidArgument("rectification matrix needs 9 values");
    for (int i = 0; i < 9; i++) p->m.dist_R[i] = p->m.rect_R[i] = v[i];
    und_init(p);
  });
}
rip_status rip_set_undistortion_projection_matrix(rip_pipeline* p, const double* v, int n) {
  return guarded(p, [&] {
    need(p);
    if (!v || n < 12) throw InvalidArgument("projection matrix needs 12 values");
    for (int i = 0; i < 12; i++) p->m.dist_P[i] = p->m.rect_P[i] = v[i];
    und_init(p);
  });
}

rip_status rip_set_tunable(rip_pipeline* p, const char* name, int value) {
  return guarded(p, [&] {
    need(p);
    if (!name) throw InvalidArgument("tunable name is null");
    if (value < 0) throw InvalidArgument("tunable values are non-negative");
    const std::string n = name;
    const rip::Tunables dflt;
    rip::Tunables& t = p->tn;
    if (n == "chain_blocks") t.chain_blocks = value;
    else if (n == "chain_frames") t.chain_frames = value;
    else if (n == "stats_blocks") t.stats_blocks = value > 0 ? value : dflt.stats_blocks;
    else if (n == "remap_ring") t.remap_ring = value;
    else if (n == "remap_stages") t.remap_stages = value > 0 ? value : dflt.remap_stages;
    else if (n == "remap_per_cu") t.remap_per_cu = value;
    else if (n == "remap_frames") t.remap_frames = value;
    else if (n == "remap_fused") t.remap_fused = value;
    else if (n == "chain_footprint") t.chain_footprint = value != 0;
    else if (n == "remap_exp") t.remap_exp = value;
    else if (n == "remap_deal") t.remap_deal = value;
    else if (n == "remap_order") t.remap_order = value <= 2 ? value : 0;
    else if (n == "chain_deal") t.chain_deal = value;
    else if (n == "chain_nt") t.chain_nt = value;
    else if (n == "remap_tiled") p->use_tiled_remap = value != 0;
    else if (n == "ccc_lds_hist_min") t.ccc_lds_hist_min = value > 0 ? value : dflt.ccc_lds_hist_min;
    else if (n == "overlap_groups") t.overlap_groups = value;
    else if (n == "overlap_mode") t.overlap_mode = value;
    else throw InvalidArgument("unknown tunable [" + n + "]");
  });
}

// ---- getters -----------------------------------------------------------------------------------
int rip_is_debayer_enabled(const rip_pipeline* p) { return p && p->m.debayer_enabled; }
int rip_is_flip_enabled(const rip_pipeline* p) { return p && p->m.flip_enabled; }
int rip_is_white_balance_enabled(const rip_pipeline* p) { return p && p->m.wb_enabled; }
int rip_is_color_calibration_enabled(const rip_pipeline* p) { return p && p->m.cc_enabled; }
int rip_is_gamma_correction_enabled(const rip_pipeline* p) { return p && p->m.gamma_enabled; }
int rip_is_vignetting_correction_enabled(const rip_pipeline* p) { return p && p->m.vig_enabled; }
int rip_is_color_enhancer_enabled(const rip_pipeline* p) { return p && p->m.ce_enabled; }
int rip_is_undistortion_enabled(const rip_pipeline* p) { return p && p->m.und_enabled; }
int rip_get_dist_image_height(const rip_pipeline* p) { return p ? p->m.dist_h : 0; }
int rip_get_dist_image_width(const rip_pipeline* p) { return p ? p->m.dist_w : 0; }
int rip_get_rect_image_height(const rip_pipeline* p) { return p ? p->m.rect_h : 0; }
int rip_get_rect_image_width(const rip_pipeline* p) { return p ? p->m.rect_w : 0; }

rip_status rip_get_debayer_method(const rip_pipeline* p, char* out, size_t cap) {
  return get_string(p, out, cap, [&] { return p->m.debayer_method; });
}
rip_status rip_get_output_format(const rip_pipeline* p, char* out, size_t cap) {
  return get_string(p, out, cap, [&] { return p->m.out().out_format; });
}
rip_status rip_get_output_yuv_matrix(const rip_pipeline* p, char* out, size_t cap) {
  return get_string(p, out, cap, [&] { return p->m.out().out_yuv_matrix; });
}
rip_status rip_get_output_interpolation(const rip_pipeline* p, char* out, size_t cap) {
  return get_string(p, out, cap, [&] { return p->m.out().out_interp; });
}
rip_status rip_get_output_fit(const rip_pipeline* p, char* out, size_t cap) {
  return get_string(p, out, cap, [&] { return p->m.out().out_fit; });
}
rip_status rip_get_dist_distortion_model(const rip_pipeline* p, char* out, size_t cap) {  // undistortion.cpp:106-112
  return get_string(p, out, cap, [&] { return p->m.und_available ? p->m.dist_model : std::string("none"); });
}
// undistortion.cpp:94-104: "none" once undistortion is enabled (the published image is rectified)
rip_status rip_get_rect_distortion_model(const rip_pipeline* p, char* out, size_t cap) {
  return get_string(p, out, cap, [&] { return p->m.und_available && !p->m.und_enabled ? p->m.rect_model : std::string("none"); });
}

rip_status rip_get_output_normalization(const rip_pipeline* p, double* divisor, double* mean, double* sd) {
  return guarded(p, [&] {
    need(p);
    if (divisor) *divisor = p->m.out().out_divisor;
    for (int i = 0; i < 3; i++) {
      if (mean) mean[i] = p->m.out().out_mean[i];
      if (sd) sd[i] = p->m.out().out_std[i];
    }
  });
}

rip_status rip_get_output_size(const rip_pipeline* p, int* width, int* height) {
  return guarded(p, [&] {
    need(p);
    if (width) *width = p->m.out().out_w;
    if (height) *height = p->m.out().out_h;
  });
}

rip_status rip_get_output_roi(const rip_pipeline* p, int* x, int* y, int* width, int* height) {
  return guarded(p, [&] {
    need(p);
    if (x) *x = p->m.out().roi_x;
    if (y) *y = p->m.out().roi_y;
    if (width) *width = p->m.out().roi_w;
    if (height) *height = p->m.out().roi_h;
  });
}

rip_status rip_get_output_pad(const rip_pipeline* p, int* b, int* g, int* r) {
  return guarded(p, [&] {
    need(p);
    if (b) *b = p->m.out().out_pad[0];
    if (g) *g = p->m.out().out_pad[1];
    if (r) *r = p->m.out().out_pad[2];
  });
}

rip_status rip_get_output_jpeg(const rip_pipeline* p, int* quality, int* restart_rows) {
  return guarded(p, [&] {
    need(p);
    if (quality) *quality = p->m.out().jpeg_quality;
    if (restart_rows) *restart_rows = p->m.out().jpeg_restart_rows;
  });
}
rip_status rip_get_output_clahe(const rip_pipeline* p, double* clip_limit, int* tiles_x, int* tiles_y) {
  return guarded(p, [&] {
    need(p);
    if (clip_limit) *clip_limit = p->m.out().clahe_clip_limit;
    if (tiles_x) *tiles_x = p->m.out().clahe_tiles_x;
    if (tiles_y) *tiles_y = p->m.out().clahe_tiles_y;
  });
}

rip_status rip_get_output_window(rip_pipeline* p, int rows, int cols, int channels, const char* encoding, int src_xywh[4], int dst_xywh[4]) {
  return guarded(p, [&] {
    need(p);
    const Plan pl = delivered_plan(p, rows, cols, channels, encoding);
    const int src[4] = {pl.win_x, pl.win_y, pl.win_w, pl.win_h}, dst[4] = {pl.pic_x, pl.pic_y, pl.pic_w, pl.pic_h};
    if (src_xywh) std::memcpy(src_xywh, src, sizeof(src));
    if (dst_xywh) std::memcpy(dst_xywh, dst, sizeof(dst));
  });
}

rip_status rip_get_output_camera_info(rip_pipeline* p, int rows, int cols, int channels, const char* encoding, int* height, int* width, double K[9],
                                      double P[12]) {
  return guarded(p, [&] {
    need(p);
    const Plan pl = delivered_plan(p, rows, cols, channels, encoding);
    const rip::Modules& m = p->m;
    double k[9], pr[12];
    for (int i = 0; i < 9; i++) k[i] = pl.remap ? m.rect_K[i] : m.dist_K[i];
    for (int i = 0; i < 12; i++) pr[i] = pl.remap ? m.rect_P[i] : m.dist_P[i];
    if (pl.fit_geometry) {
      // the same mapping from the window that is read to the picture's rectangle: u = (u' - left + 0.5) / a - 0.5 + xs (PARITY.md
      // "Resize: window and fit"); every operation rounded, in this order
      const double a = (double)pl.pic_w / pl.win_w, b = (double)pl.pic_h / pl.win_h;
      const double xs = pl.win_x, ys = pl.win_y, left = pl.pic_x, top = pl.pic_y;
      k[0] *= a;
      k[1] *= a;
      k[2] = (a * ((k[2] - xs) + 0.5) - 0.5) + left;
      k[4] *= b;
      k[5] = (b * ((k[5] - ys) + 0.5) - 0.5) + top;
      pr[0] *= a;
      pr[1] *= a;
      pr[2] = (a * ((pr[2] - xs) + 0.5) - 0.5) + left;
      pr[3] *= a;
      pr[5] *= b;
      pr[6] = (b * ((pr[6] - ys) + 0.5) - 0.5) + top;
      pr[7] *= b;
    } else if (pl.rsz_active) {
      // the inverse of the tables' pixel-centre mapping u = (u' + 0.5) / a - 0.5 (PARITY.md "Resize")
      const double a = (double)pl.dl_pic_cols / pl.out_cols, b = (double)pl.img_rows / pl.out_rows;
      k[0] *= a;
      k[1] *= a;
      k[2] = a * (k[2] + 0.5) - 0.5;
      k[4] *= b;
      k[5] = b * (k[5] + 0.5) - 0.5;
      pr[0] *= a;
      pr[1] *= a;
      pr[2] = a * (pr[2] + 0.5) - 0.5;
      pr[3] *= a;
      pr[5] *= b;
      pr[6] = b * (pr[6] + 0.5) - 0.5;
      pr[7] *= b;
    }
    if (height) *height = pl.img_rows;  // the picture, not the buffer a YUV format delivers it in
    if (width) *width = pl.dl_pic_cols;
    if (K) std::memcpy(K, k, sizeof(k));
    if (P) std::memcpy(P, pr, sizeof(pr));
  });
}

rip_status rip_get_debayer_16bit_range(const rip_pipeline* p, int* black, int* white) {
  return guarded(p, [&] {
    need(p);
    if (black) *black = p->m.raw16_black;
    if (white) *white = p->m.raw16_white;
  });
}

rip_status rip_get_color_calibration_matrix(const rip_pipeline* p, double* out) { return get_vec(p, out, p ? p->m.cc_matrix : nullptr, 9); }
rip_status rip_get_color_calibration_bias(const rip_pipeline* p, double* out) { return get_vec(p, out, p ? p->m.cc_bias : nullptr, 4); }
rip_status rip_get_dist_camera_matrix(const rip_pipeline* p, double* out) { return get_vec(p, out, p ? p->m.dist_K : nullptr, 9); }
rip_status rip_get_dist_distortion_coefficients(const rip_pipeline* p, double* out) { return get_vec(p, out, p ? p->m.dist_D : nullptr, 4); }
rip_status rip_get_dist_rectification_matrix(const rip_pipeline* p, double* out) { return get_vec(p, out, p ? p->m.dist_R : nullptr, 9); }
rip_status rip_get_dist_projection_matrix(const rip_pipeline* p, double* out) { return get_vec(p, out, p ? p->m.dist_P : nullptr, 12); }
rip_status rip_get_rect_camera_matrix(const rip_pipeline* p, double* out) { return get_vec(p, out, p ? p->m.rect_K : nullptr, 9); }
rip_status rip_get_rect_distortion_coefficients(const rip_pipeline* p, double* out) { return get_vec(p, out, p ? p->m.rect_D : nullptr, 4); }
rip_status rip_get_rect_rectification_matrix(const rip_pipeline* p, double* out) { return get_vec(p, out, p ? p->m.rect_R : nullptr, 9); }
rip_status rip_get_rect_projection_matrix(const rip_pipeline* p, double* out) { return get_vec(p, out, p ? p->m.rect_P : nullptr, 12); }

rip_status rip_get_distortion_coefficients_n(const rip_pipeline* p, int rect, double* out, int capacity, int* n) {
  return guarded(p, [&] {
    need(p);
    if (rect != 0 && rect != 1) throw InvalidArgument("rect must be 0 (dist) or 1 (rect)");
    const rip::Modules& m = p->m;
    const int count = rip::distortion_coefficient_count(rect ? m.rect_model : m.dist_model);
    if (n) *n = count;
    if (!out) return;  // the count alone
    if (capacity < count) throw CapacityError("coefficient buffer too small");
    if (rect) {
      for (int i = 0; i < count; i++) out[i] = m.rect_D[i];
    } else if (rip::is_pinhole_model(m.dist_model)) {
      double k[8];
      rip::pinhole_coefficients(m.dist_model, m.dist_D, k);  // what the model evaluates: radtan reports k3 = 0
      for (int i = 0; i < count; i++) out[i] = k[i];
    } else {
      for (int i = 0; i < count; i++) out[i] = m.dist_D[i];
    }
  });
}

}  // extern "C"
#pragma GCC visibility pop
