// rip_params.hpp -- the module parameters of one pipeline (mirroring the reference's eight modules, plus the output heads), their
// loaders and example values, and the check or name -> id function of every setting.  check_output_normalization is the one check
// that lives elsewhere: build_output_table applies it itself, so it stands next to it in rip_output_tables.hpp.
#pragma once
#include <string>

namespace rip {

// ---------------------------------------------------------------------------------------------
// Module parameters.  Field comments cite the reference member they mirror.
// ---------------------------------------------------------------------------------------------
// One output head (rip_set_output_heads; PARITY.md "Output heads"): one complete set of the output stage's settings.  A handle holds
// up to kMaxOutputHeads of them; head 0 is the output of a handle that never asked for more.
constexpr int kMaxOutputHeads = 8;
struct OutputHead {
  // extension (rip_set_output_format, rip_set_output_normalization): the output stage behind the last module -- the format the
  // frame calls deliver ("native": the pipeline's own image) and the normalisation of the planar float formats, mean / std in
  // the order of the format's planes
  std::string out_format = "native";
  // extension (rip_set_output_yuv_matrix): the matrix and range of the formats "nv12" / "i420"; without effect under any other format
  std::string out_yuv_matrix = "bt601";
  double out_divisor = 255.0, out_mean[3] = {0, 0, 0}, out_std[3] = {1, 1, 1};
  // extension (rip_set_output_size): the size the delivered frames are resized to, in front of the output format; (0, 0) = off
  int out_w = 0, out_h = 0;
  // extension (rip_set_output_interpolation): the filter of that resize, "linear", "area", "linear_aa" or "cubic_aa"; without effect while no target is active
  std::string out_interp = "linear";
  // extension (rip_set_output_roi, rip_set_output_fit, rip_set_output_pad; PARITY.md "Resize: window and fit"): the window of the
  // final image the resize stage reads ((0, 0, 0, 0) = all of it), how the window is placed in the target ("stretch", "letterbox",
  // "crop"; without effect while no target is active) and the colour (B, G, R) of what a letterbox leaves uncovered
  int roi_x = 0, roi_y = 0, roi_w = 0, roi_h = 0;
  std::string out_fit = "stretch";
  int out_pad[3] = {114, 114, 114};
  // extension (rip_set_output_clahe; PARITY.md "Local contrast: CLAHE"): cv::CLAHE on the delivered one-channel picture, the last
  // launch of the head; tiles (0, 0) = off
  double clahe_clip_limit = 0.0;
  int clahe_tiles_x = 0, clahe_tiles_y = 0;
  // extension (rip_set_output_jpeg; PARITY.md "Output formats: JPEG"): the quality (1..100, the IJG scaling of the Annex K tables) and
  // the MCU rows per restart interval (1..64) of the format "jpeg"; without effect under any other format
  int jpeg_quality = 90, jpeg_restart_rows = 1;
};

struct Modules {
  bool use_gpu = false, debug = false;
  // DebayerModule (debayer.hpp:70-72): enable flag stored but ignored by apply (:38-40)
  bool debayer_enabled = true;
  std::string debayer_encoding = "auto";
  bool debayer_16bit = false;  // extension (rip_set_debayer_16bit): accept bayer_*16 instead of throwing like the reference
  // extension (rip_set_debayer_16bit_range): black and white level of bayer_*16 frames; (0, 0) = off (bgr16 out, no other
  // stage); 0 <= black < white <= 65535: narrowed to 8 bits right after the demosaic, then the whole chain (PARITY.md)
  int raw16_black = 0, raw16_white = 0;
  // extension (rip_set_debayer_method): "bilinear" (the CPU path, debayer.cpp:49-70) or "mht" (Malvar-He-Cutler, what the
  // CUDA path's cv::cuda::demosaicing(..., COLOR_Bayer**2BGR_MHT) computes, debayer.cpp:93-108)
  std::string debayer_method = "bilinear";
  // extension (rip_set_output_heads, rip_select_output_head): the output stage's settings, one set per head; heads at and beyond
  // n_heads hold the defaults.  The single-output calls read and write the selected head through out().
  OutputHead heads[kMaxOutputHeads];
  int n_heads = 1, selected = 0;
  OutputHead& out() { return heads[selected]; }
  const OutputHead& out() const { return heads[selected]; }
  // FlipModule (flip.hpp:63-66)
  bool flip_enabled = false;
  int flip_angle = 0;
  // WhiteBalanceModule (white_balance.hpp:108-116)
  bool wb_enabled = false;
  std::string wb_method = "ccc";
  double wb_percentile = 20.0, wb_bright_thr = 0.8, wb_dark_thr = 0.1;
  bool wb_temporal = true;
  // ColorCalibrationModule (color_calibration.hpp:76-81): matrix held as Matx33f
  bool cc_enabled = false, cc_available = false;
  float cc_matrix[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double cc_bias[4] = {0, 0, 0, 0};
  // GammaCorrectionModule (gamma_correction.hpp:66-70)
  bool gamma_enabled = false;
  std::string gamma_method = "custom";
  double gamma_k = 1.0;
  // VignettingCorrectionModule (vignetting_correction.hpp:52-55)
  bool vig_enabled = false;
  double vig_scale = 1.5, vig_a2 = 1e-3, vig_a4 = 1e-6;
  // ColorEnhancerModule (color_enhancer.hpp:58-60): members, after the cross-wired setters
  bool ce_enabled = false;
  double ce_value_gain = 1.0, ce_saturation_gain = 1.0, ce_hue_gain = 1.0;
  // UndistortionModule (undistortion.hpp:100-125)
  bool und_enabled = false, und_available = false;
  std::string dist_model = "none", rect_model = "none";
  double dist_K[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, rect_K[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  // as given (up to 8, the rest 0): the fisheye builder reads the first four, the pinhole models what pinhole_coefficients() keeps
  double dist_D[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rect_D[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double dist_R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, rect_R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double dist_P[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, rect_P[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  int dist_w = 320, dist_h = 240, rect_w = 320, rect_h = 240;
  double balance = 0.0, fov_scale = 1.0;
  // extension (rip_set_rect_mask; PARITY.md "Rect mask"): "off", "coverage" or "valid" -- what RIP_IMAGE_RECT_MASK and
  // rip_get_output_mask hand out.  The frame calls never look at it.
  std::string rect_mask = "off";
};
// the mask modes rip_set_rect_mask accepts: 0 "off", 1 "coverage", 2 "valid"; throws std::invalid_argument naming them otherwise
int rect_mask_mode_id(const std::string& name);

// Parameter loaders (throw YamlError on malformed files; a missing file is a soft failure
// that returns false, as the reference's std::cout warning paths do).
void apply_example_params(Modules& m);  // the values of config/pipeline_params_example.yaml
bool load_params_file(Modules& m, const std::string& path);             // raw_image_pipeline.cpp:44-165
// the demosaic methods rip_set_debayer_method accepts; throws std::invalid_argument naming them for any other name
void check_debayer_method(const std::string& method);
// the 16-bit ranges rip_set_debayer_16bit_range accepts: (0, 0) or 0 <= black < white <= 65535; throws std::invalid_argument
void check_debayer_16bit_range(int black, int white);
// the output formats rip_set_output_format accepts: the id (rip_output.hpp OutputFormat; 0 = "native"); throws
// std::invalid_argument listing the names for any other name
int output_format_id(const std::string& name);
// the matrices rip_set_output_yuv_matrix accepts: 0 "bt601", 1 "bt709", 2 "bt601_full", 3 "bt709_full"; throws std::invalid_argument
// listing the names otherwise
int output_yuv_matrix_id(const std::string& name);
// the target sizes rip_set_output_size accepts: (0, 0), or both in 1 .. 16384; throws std::invalid_argument naming the rule
void check_output_size(int width, int height);
// the names rip_set_output_interpolation accepts: 0 for "linear", 1 for "area", 2 for "linear_aa", 3 for "cubic_aa"; throws
// std::invalid_argument naming them otherwise
int output_interpolation_id(const std::string& name);
// the windows rip_set_output_roi accepts: (0, 0, 0, 0), or x, y >= 0 with width and height in 1 .. 16384; throws std::invalid_argument
void check_output_roi(int x, int y, int width, int height);
// the names rip_set_output_fit accepts: 0 for "stretch", 1 for "letterbox", 2 for "crop"; throws std::invalid_argument naming them otherwise
int output_fit_id(const std::string& name);
// the pad colours rip_set_output_pad accepts: every component in 0 .. 255; throws std::invalid_argument
void check_output_pad(int b, int g, int r);
// the settings rip_set_output_clahe accepts: a finite clip limit >= 0 and tiles both in 1 .. 16 or both 0; throws std::invalid_argument
void check_output_clahe(double clip_limit, int tiles_x, int tiles_y);
// the settings rip_set_output_jpeg accepts: a quality in 1 .. 100 and 1 .. 64 MCU rows per restart interval; throws std::invalid_argument
void check_output_jpeg(int quality, int restart_rows);
bool load_camera_calibration_file(Modules& m, const std::string& path); // undistortion.cpp:157-195
bool load_color_calibration_file(Modules& m, const std::string& path);  // color_calibration.cpp:52-76
void apply_example_camera_calibration(Modules& m);  // values of config/alphasense_calib_example.yaml
void apply_example_color_calibration(Modules& m);   // values of config/alphasense_color_calib_example.yaml

}  // namespace rip
