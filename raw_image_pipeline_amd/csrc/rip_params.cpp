// rip_params.cpp -- parameter loaders, example values and the checks of the settings (rip_params.hpp).
#include "rip_params.hpp"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <vector>

#include "rip_output_tables.hpp"
#include "rip_yaml.hpp"

namespace rip {

// =============================================================================================
// Parameter loaders
// =============================================================================================
namespace {
void set_enhancer_gains_from_config(Modules& m, double hue, double sat, double val) {
  // Through the public setters (color_enhancer.cpp:23-33): setHueGain -> value_gain_,
  // setSaturationGain -> saturation_gain_, setValueGain -> hue_gain_.  The reference's YAML
  // loader calls setHueGain three times (raw_image_pipeline.cpp:143-145) and leaves two
  // members uninitialised; here each key goes through its own setter (documented fix, Q7).
  m.ce_value_gain = hue;
  m.ce_saturation_gain = sat;
  m.ce_hue_gain = val;
}

// One section of output settings (output:, output_1: .. output_7:; `sec` names it in the messages): every key checked before anything
// is handed back, so an invalid value fails the load and leaves every parameter as it was.
OutputHead output_head_from_node(const YamlNode& o, const std::string& sec) {
  // extension keys output: format: / divisor: / mean: [3] / std: [3] (rip_set_output_format, rip_set_output_normalization);
  // absent keys mean the defaults, an invalid value fails the load like an unknown debayer method
  const std::string out_format = o.get("format", std::string("native"));
  (void)output_format_id(out_format);
  // extension key output: yuv_matrix: bt601 | bt709 | bt601_full | bt709_full (rip_set_output_yuv_matrix); absent means bt601
  const std::string out_yuv_matrix = o.get("yuv_matrix", std::string("bt601"));
  (void)output_yuv_matrix_id(out_yuv_matrix);
  if (o["yuv_matrix"].defined() && o["yuv_matrix"].kind != YamlNode::Scalar)
    throw std::invalid_argument(sec + ": yuv_matrix: one word is expected, \"bt601\", \"bt709\", \"bt601_full\" or \"bt709_full\"");
  const double out_divisor = o.get("divisor", 255.0);
  double out_mean[3] = {0, 0, 0}, out_std[3] = {1, 1, 1};
  for (int which = 0; which < 2; which++) {
    const char* key = which ? "std" : "mean";
    if (!o[key].defined()) continue;
    const std::vector<double> v = o.get_vector(key);
    if (v.size() != 3) throw std::invalid_argument(sec + ": " + key + ": a sequence of 3 numbers is expected");
    for (int i = 0; i < 3; i++) (which ? out_std : out_mean)[i] = v[i];
  }
  check_output_normalization(out_divisor, out_mean, out_std);
  // extension key output: size: [width, height] (rip_set_output_size); absent means off
  int out_w = 0, out_h = 0;
  if (o["size"].defined()) {
    const std::vector<double> v = o.get_vector("size");
    if (v.size() != 2 || !(v[0] >= 0 && v[0] <= 16384 && v[1] >= 0 && v[1] <= 16384) || v[0] != std::floor(v[0]) || v[1] != std::floor(v[1]))
      throw std::invalid_argument(sec + ": size: a sequence [width, height] of two integers in 1..16384 (or [0, 0]) is expected");
    out_w = (int)v[0];
    out_h = (int)v[1];
    check_output_size(out_w, out_h);
  }
  // extension key output: interpolation: linear | area | linear_aa | cubic_aa (rip_set_output_interpolation); absent means linear
  const std::string out_interp = o.get("interpolation", std::string("linear"));
  (void)output_interpolation_id(out_interp);
  if (o["interpolation"].defined() && o["interpolation"].kind != YamlNode::Scalar)
    throw std::invalid_argument(sec + ": interpolation: one word is expected, \"linear\" or \"area\", \"linear_aa\" or \"cubic_aa\"");
  // extension keys output: roi: [x, y, w, h] / fit: stretch | letterbox | crop / pad: [b, g, r] (rip_set_output_roi,
  // rip_set_output_fit, rip_set_output_pad); absent keys mean the defaults
  int roi[4] = {0, 0, 0, 0}, pad[3] = {114, 114, 114};
  for (int which = 0; which < 2; which++) {
    const char* key = which ? "pad" : "roi";
    const size_t n = which ? 3 : 4;
    if (!o[key].defined()) continue;
    const std::vector<double> v = o.get_vector(key);
    bool ok = v.size() == n;
    for (size_t i = 0; ok && i < n; i++) ok = v[i] >= 0 && v[i] <= (1 << 22) && v[i] == std::floor(v[i]);
    if (!ok)
      throw std::invalid_argument(which ? sec + ": pad: a sequence [b, g, r] of three integers in 0..255 is expected"
                                        : sec + ": roi: a sequence [x, y, width, height] of four integers is expected, x and y at least 0, width and height in 1..16384 (or four zeros)");
    for (size_t i = 0; i < n; i++) (which ? pad : roi)[i] = (int)v[i];
  }
  check_output_roi(roi[0], roi[1], roi[2], roi[3]);
  check_output_pad(pad[0], pad[1], pad[2]);
  const std::string out_fit = o.get("fit", std::string("stretch"));
  (void)output_fit_id(out_fit);
  if (o["fit"].defined() && o["fit"].kind != YamlNode::Scalar)
    throw std::invalid_argument(sec + ": fit: one word is expected, \"stretch\", \"letterbox\" or \"crop\"");
  // extension keys output: clahe_clip_limit: 3.0 / clahe_tiles: [tiles_x, tiles_y] (rip_set_output_clahe); absent keys mean off
  const double clahe_clip_limit = o.get("clahe_clip_limit", 0.0);
  int clahe_tiles[2] = {0, 0};
  if (o["clahe_tiles"].defined()) {
    const std::vector<double> v = o.get_vector("clahe_tiles");
    if (v.size() != 2 || !(v[0] >= 0 && v[0] <= 16 && v[1] >= 0 && v[1] <= 16) || v[0] != std::floor(v[0]) || v[1] != std::floor(v[1]))
      throw std::invalid_argument(sec + ": clahe_tiles: a sequence [tiles_x, tiles_y] of two integers in 1..16 (or [0, 0]) is expected");
    clahe_tiles[0] = (int)v[0];
    clahe_tiles[1] = (int)v[1];
  }
  check_output_clahe(clahe_clip_limit, clahe_tiles[0], clahe_tiles[1]);
  // extension keys output: jpeg_quality: 90 / jpeg_restart_rows: 1 (rip_set_output_jpeg); absent keys mean the defaults
  const double jpeg_quality = o.get("jpeg_quality", 90.0), jpeg_restart_rows = o.get("jpeg_restart_rows", 1.0);
  if (jpeg_quality != std::floor(jpeg_quality) || jpeg_restart_rows != std::floor(jpeg_restart_rows) || !(std::fabs(jpeg_quality) < 1e6) || !(std::fabs(jpeg_restart_rows) < 1e6))
    throw std::invalid_argument(sec + ": jpeg_quality: an integer in 1..100 and jpeg_restart_rows: an integer in 1..64 are expected");
  check_output_jpeg((int)jpeg_quality, (int)jpeg_restart_rows);
  OutputHead h;
  h.jpeg_quality = (int)jpeg_quality, h.jpeg_restart_rows = (int)jpeg_restart_rows;
  h.clahe_clip_limit = clahe_clip_limit;
  h.clahe_tiles_x = clahe_tiles[0], h.clahe_tiles_y = clahe_tiles[1];
  h.roi_x = roi[0], h.roi_y = roi[1], h.roi_w = roi[2], h.roi_h = roi[3];
  h.out_fit = out_fit;
  for (int i = 0; i < 3; i++) h.out_pad[i] = pad[i];
  h.out_w = out_w;
  h.out_h = out_h;
  h.out_interp = out_interp;
  h.out_format = out_format;
  h.out_yuv_matrix = out_yuv_matrix;
  h.out_divisor = out_divisor;
  for (int i = 0; i < 3; i++) h.out_mean[i] = out_mean[i], h.out_std[i] = out_std[i];
  return h;
}

void params_from_node(Modules& m, const YamlNode& node) {
  // extension key debayer: method: (not in the reference's files).  Checked before anything is assigned: an unknown method
  // fails the load and leaves every parameter as it was.
  const std::string debayer_method = node["debayer"].get("method", std::string("bilinear"));
  check_debayer_method(debayer_method);
  // extension keys debayer: accept_16bit: / black_level: / white_level: (rip_set_debayer_16bit, rip_set_debayer_16bit_range);
  // loadParams re-creates the modules, so absent keys mean off.  An invalid range fails the load like an unknown method.
  const int black_level = node["debayer"].get("black_level", 0), white_level = node["debayer"].get("white_level", 0);
  check_debayer_16bit_range(black_level, white_level);
  // extension key undistortion: mask: (rip_set_rect_mask); an absent key means off, an unknown word fails the load
  const std::string rect_mask = node["undistortion"].get("mask", std::string("off"));
  (void)rect_mask_mode_id(rect_mask);
  if (node["undistortion"]["mask"].defined() && node["undistortion"]["mask"].kind != YamlNode::Scalar)
    throw std::invalid_argument("undistortion: mask: one word is expected, \"off\", \"coverage\" or \"valid\"");
  // extension keys output: ... (output_head_from_node) and the further heads' sections output_1: .. output_7: with the same keys
  // (rip_set_output_heads): n = 1 + the largest k present, sections absent in between hold the defaults, head 0 is selected
  OutputHead heads[kMaxOutputHeads];
  int n_heads = 1;
  heads[0] = output_head_from_node(node["output"], "output");
  for (const auto& kv : node.map) {
    if (kv.first.compare(0, 7, "output_") != 0) continue;
    const std::string idx = kv.first.substr(7);
    if (idx.size() != 1 || idx[0] < '1' || idx[0] > '0' + kMaxOutputHeads - 1)
      throw std::invalid_argument(kv.first + ": the sections of further output heads are output_1 .. output_" + std::to_string(kMaxOutputHeads - 1));
    const int k = idx[0] - '0';
    heads[k] = output_head_from_node(kv.second, kv.first);
    n_heads = std::max(n_heads, k + 1);
  }
  for (int k = 0; k < kMaxOutputHeads; k++) m.heads[k] = heads[k];
  m.n_heads = n_heads;
  m.selected = 0;
  m.debayer_method = debayer_method;
  m.debayer_16bit = node["debayer"].get("accept_16bit", false);
  m.raw16_black = black_level;
  m.raw16_white = white_level;
  // raw_image_pipeline.cpp:54-160, defaults as written there
  m.debayer_enabled = node["debayer"].get("enabled", true);
  m.debayer_encoding = node["debayer"].get("encoding", std::string("auto"));
  m.flip_enabled = node["flip"].get("enabled", false);
  m.flip_angle = node["flip"].get("angle", 0);
  const YamlNode& wb = node["white_balance"];
  m.wb_enabled = wb.get("enabled", false);
  m.wb_method = wb.get("method", std::string("ccc"));
  m.wb_percentile = wb.get("clipping_percentile", 20.0);
  m.wb_bright_thr = wb.get("saturation_bright_thr", 0.8);
  m.wb_dark_thr = wb.get("saturation_dark_thr", 0.1);
  m.wb_temporal = wb.get("temporal_consistency", true);
  m.cc_enabled = node["color_calibration"].get("enabled", false);
  const YamlNode& g = node["gamma_correction"];
  m.gamma_enabled = g.get("enabled", false);
  m.gamma_method = g.get("method", std::string("custom"));
  m.gamma_k = g.get("k", 0.8);
  const YamlNode& v = node["vignetting_correction"];
  m.vig_enabled = v.get("enabled", false);
  m.vig_scale = v.get("scale", 1.5);
  m.vig_a2 = v.get("a2", 1e-3);
  m.vig_a4 = v.get("a4", 1e-6);
  const YamlNode& ce = node["color_enhancer"];
  m.ce_enabled = ce.get("run_color_enhancer", false);  // key name as in the reference (:137)
  set_enhancer_gains_from_config(m, ce.get("hue_gain", 1.0), ce.get("saturation_gain", 1.0), ce.get("value_gain", 1.0));
  const YamlNode& u = node["undistortion"];
  m.und_enabled = u.get("enabled", false);
  m.balance = u.get("balance", 0.0);
  m.fov_scale = u.get("fov_scale", 1.0);
  m.rect_mask = rect_mask;
}

void set_camera(Modules& m, int w, int h, const std::vector<double>& K, const std::vector<double>& D,
                const std::string& model, const std::vector<double>& R, const std::vector<double>& P) {
  // the six setters of undistortion.cpp:23-72, each of which writes both the dist_ and rect_ copy
  m.dist_w = m.rect_w = w;
  m.dist_h = m.rect_h = h;
  if (K.size() < 9 || D.size() < 4 || R.size() < 9 || P.size() < 12)
    throw YamlError("camera calibration: camera_matrix needs 9, distortion_coefficients 4, rectification_matrix 9 and projection_matrix 12 values");
  // ROS's 12 / 14-value vectors (thin-prism s1..s4, tilt tauX tauY) load as long as those terms are zero
  for (size_t i = 8; i < D.size(); i++)
    if (D[i] != 0)
      throw std::invalid_argument("camera calibration: distortion_coefficients has " + std::to_string(D.size()) +
                                  " values with a non-zero thin-prism / tilt term (value " + std::to_string(i + 1) +
                                  "); only k1 k2 p1 p2 k3 k4 k5 k6 are supported");
  for (int i = 0; i < 9; i++) m.dist_K[i] = m.rect_K[i] = K[i];
  for (int i = 0; i < 8; i++) m.dist_D[i] = m.rect_D[i] = i < (int)D.size() ? D[i] : 0.0;
  m.dist_model = m.rect_model = model;
  for (int i = 0; i < 9; i++) m.dist_R[i] = m.rect_R[i] = R[i];
  for (int i = 0; i < 12; i++) m.dist_P[i] = m.rect_P[i] = P[i];
}
}  // namespace

void apply_example_params(Modules& m) {
  // values of the reference's config/pipeline_params_example.yaml (facts, not text)
  m.debayer_enabled = true;
  m.debayer_encoding = "auto";
  m.debayer_method = "bilinear";
  m.flip_enabled = false;
  m.flip_angle = 0;
  m.wb_enabled = true;
  m.wb_method = "ccc";
  m.wb_percentile = 20;
  m.wb_bright_thr = 0.8;
  m.wb_dark_thr = 0.2;
  m.wb_temporal = false;
  m.cc_enabled = false;
  m.gamma_enabled = false;
  m.gamma_method = "custom";
  m.gamma_k = 0.8;
  m.vig_enabled = false;
  m.vig_scale = 1.5;
  m.vig_a2 = 1e-3;
  m.vig_a4 = 1e-6;
  m.ce_enabled = false;
  set_enhancer_gains_from_config(m, 1.0, 1.5, 1.0);
  m.und_enabled = true;
  m.balance = 0.0;
  m.fov_scale = 0.8;
}

int rect_mask_mode_id(const std::string& name) {
  if (name == "off") return 0;
  if (name == "coverage") return 1;
  if (name == "valid") return 2;
  throw std::invalid_argument("Rect mask mode [" + name + "] not supported. Supported modes: 'off', 'coverage', 'valid'");
}

void check_debayer_method(const std::string& method) {
  if (method != "bilinear" && method != "mht")
    throw std::invalid_argument("Debayer method [" + method + "] not supported. Supported methods: 'bilinear', 'mht'");
}

namespace {
const char* const kOutputFormatNames[12] = {"native", "rgb8", "mono8", "rgb_chw_f32", "rgb_chw_f16", "rgb_chw_bf16",
                                            "bgr_chw_f32", "bgr_chw_f16", "bgr_chw_bf16", "nv12", "i420", "jpeg"};  // index = rip_output.hpp OutputFormat
// index = the id output_yuv_matrix_id returns; the rows are rip_yuv.hpp's YuvMatrix (PARITY.md "Output formats: YUV 4:2:0")
const char* const kYuvMatrixNames[4] = {"bt601", "bt709", "bt601_full", "bt709_full"};
}  // namespace

int output_format_id(const std::string& name) {
  std::string names;
  for (int i = 0; i < 12; i++) {
    if (name == kOutputFormatNames[i]) return i;
    names += std::string(i ? ", '" : "'") + kOutputFormatNames[i] + "'";
  }
  throw std::invalid_argument("Output format [" + name + "] not supported. Supported formats: " + names);
}

int output_yuv_matrix_id(const std::string& name) {
  std::string names;
  for (int i = 0; i < 4; i++) {
    if (name == kYuvMatrixNames[i]) return i;
    names += std::string(i ? ", '" : "'") + kYuvMatrixNames[i] + "'";
  }
  throw std::invalid_argument("Output YUV matrix [" + name + "] not supported. Supported matrices: " + names);
}

void check_output_size(int width, int height) {
  if (width == 0 && height == 0) return;  // off
  if (width < 1 || height < 1 || width > 16384 || height > 16384)
    throw std::invalid_argument("output size (" + std::to_string(width) + ", " + std::to_string(height) +
                                ") not supported: (0, 0) switches it off, otherwise width and height are both in 1..16384");
}

void check_output_roi(int x, int y, int width, int height) {
  if (x == 0 && y == 0 && width == 0 && height == 0) return;  // off
  if (x < 0 || y < 0 || width < 1 || height < 1 || width > 16384 || height > 16384)
    throw std::invalid_argument("output roi (" + std::to_string(x) + ", " + std::to_string(y) + ", " + std::to_string(width) + ", " + std::to_string(height) +
                                ") not supported: (0, 0, 0, 0) switches it off, otherwise x and y are at least 0 and width and height are in 1..16384");
}

int output_fit_id(const std::string& name) {
  if (name == "stretch") return 0;
  if (name == "letterbox") return 1;
  if (name == "crop") return 2;
  throw std::invalid_argument("output fit \"" + name + "\" not supported: \"stretch\", \"letterbox\" or \"crop\"");
}

void check_output_pad(int b, int g, int r) {
  for (int v : {b, g, r})
    if (v < 0 || v > 255)
      throw std::invalid_argument("output pad (" + std::to_string(b) + ", " + std::to_string(g) + ", " + std::to_string(r) + ") not supported: every component is in 0..255");
}

void check_output_clahe(double clip_limit, int tiles_x, int tiles_y) {
  if (!std::isfinite(clip_limit) || clip_limit < 0)
    throw std::invalid_argument("output clahe: the clip limit must be finite and at least 0 (0: no clipping), got " + std::to_string(clip_limit));
  const bool off = tiles_x == 0 && tiles_y == 0;
  if (!off && (tiles_x < 1 || tiles_x > 16 || tiles_y < 1 || tiles_y > 16))
    throw std::invalid_argument("output clahe: tiles (" + std::to_string(tiles_x) + ", " + std::to_string(tiles_y) + ") not supported: both in 1..16, or (0, 0) for off");
}

void check_output_jpeg(int quality, int restart_rows) {
  if (quality < 1 || quality > 100 || restart_rows < 1 || restart_rows > 64)
    throw std::invalid_argument("output jpeg (quality " + std::to_string(quality) + ", restart rows " + std::to_string(restart_rows) +
                                ") not supported: the quality is in 1..100 and the MCU rows per restart interval are in 1..64");
}

int output_interpolation_id(const std::string& name) {
  if (name == "linear") return 0;
  if (name == "area") return 1;
  if (name == "linear_aa") return 2;
  if (name == "cubic_aa") return 3;
  throw std::invalid_argument("output interpolation \"" + name + "\" not supported: \"linear\" or \"area\", \"linear_aa\" or \"cubic_aa\"");
}

void check_debayer_16bit_range(int black, int white) {
  if (black == 0 && white == 0) return;  // off
  if (black < 0 || white > 65535 || black >= white)
    throw std::invalid_argument("16-bit range (" + std::to_string(black) + ", " + std::to_string(white) +
                                ") not supported: (0, 0) switches it off, otherwise 0 <= black < white <= 65535");
}

bool load_params_file(Modules& m, const std::string& path) {
  if (!file_exists(path)) return false;  // "Warning: parameters file doesn't exist" (:162-164)
  params_from_node(m, yaml_load_file(path));
  return true;
}

bool load_camera_calibration_file(Modules& m, const std::string& path) {
  if (!file_exists(path)) {
    // undistortion.cpp:175-194
    m.und_available = false;
    set_camera(m, 320, 240, {1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0, 0}, "none", {1, 0, 0, 0, 1, 0, 0, 0, 1},
               {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0});
    return false;
  }
  YamlNode n = yaml_load_file(path);
  set_camera(m, n.get("image_width", 320), n.get("image_height", 240), n["camera_matrix"].get_vector("data"),
             n["distortion_coefficients"].get_vector("data"), n.get("distortion_model", std::string("none")),
             n["rectification_matrix"].get_vector("data"), n["projection_matrix"].get_vector("data"));
  m.und_available = true;
  return true;
}

bool load_color_calibration_file(Modules& m, const std::string& path) {
  if (!file_exists(path)) {
    m.cc_available = false;  // color_calibration.cpp:72-75
    return false;
  }
  YamlNode n = yaml_load_file(path);
  std::vector<double> mat = n["matrix"].get_vector("data");
  std::vector<double> bias = n["bias"].get_vector("data");
  if (mat.size() != 9) mat = {1, 0, 0, 0, 1, 0, 0, 0, 1};  // utils::get default on decode failure
  if (bias.size() != 3) bias = {0, 0, 0};
  for (int i = 0; i < 9; i++) m.cc_matrix[i] = (float)mat[i];  // Matx33d -> Matx33f (:79)
  for (int i = 0; i < 3; i++) m.cc_bias[i] = bias[i];
  m.cc_bias[3] = 0;
  m.cc_available = true;
  return true;
}

void apply_example_camera_calibration(Modules& m) {
  // values of config/alphasense_calib_example.yaml
  set_camera(m, 720, 540,
             {347.548139773951, 0.0, 342.454373227748, 0.0, 347.434712422309, 271.368057185649, 0.0, 0.0, 1.0},
             {-0.0396482888762527, -0.00367688950406141, 0.00391742438164282, -0.00178738156007817}, "equidistant",
             {1, 0, 0, 0, 1, 0, 0, 0, 1},
             {347.548139773951, 0.0, 342.454373227748, 0.0, 0.0, 347.434712422309, 271.368057185649, 0.0, 0.0, 0.0, 1.0, 0.0});
  m.und_available = true;
}

void apply_example_color_calibration(Modules& m) {
  // values of config/alphasense_color_calib_example.yaml
  const double mat[9] = {2.4276948, 0.21479778, -0.30818, 0.09277014, 1.1962607, -0.09772757, -0.24436986, -0.22239459, 2.099912};
  for (int i = 0; i < 9; i++) m.cc_matrix[i] = (float)mat[i];
  for (int i = 0; i < 4; i++) m.cc_bias[i] = 0;
  m.cc_available = true;
}

}  // namespace rip
