// rip_host.hpp -- host-side state of one pipeline: module parameters (mirroring the reference's
// eight modules), the YAML-subset reader for the three config files, and the builders of the
// constant tables / undistortion maps the HIP kernels consume.  No device code here.
#pragma once
#include "rip_tile.hpp"

#include <cstdint>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace rip {

// ---------------------------------------------------------------------------------------------
// Minimal YAML reader: nested block maps, scalars, flow sequences of scalars ("[a, b, c]",
// possibly spanning lines), comments.  Enough for the reference's three file kinds
// (config/pipeline_params_example.yaml, alphasense_calib_example.yaml,
// alphasense_color_calib_example.yaml).  Throws YamlError on malformed input.
// ---------------------------------------------------------------------------------------------
struct YamlError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

struct YamlNode {
  enum Kind { Null, Scalar, Sequence, Map } kind = Null;
  std::string scalar;
  std::vector<std::string> seq;
  std::map<std::string, YamlNode> map;

  const YamlNode& operator[](const std::string& key) const;  // Null node when absent
  bool defined() const { return kind != Null; }
  // utils::get<T>(node, key, default) (reference utils.hpp:61-74): value or default
  bool get(const std::string& key, bool dflt) const;
  int get(const std::string& key, int dflt) const;
  double get(const std::string& key, double dflt) const;
  std::string get(const std::string& key, const std::string& dflt) const;
  std::vector<double> get_vector(const std::string& key) const;  // empty when absent / not a sequence
};
YamlNode yaml_parse(const std::string& text);
YamlNode yaml_load_file(const std::string& path);  // throws YamlError when unreadable
bool file_exists(const std::string& path);

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
// the integers of matrix `id` (PARITY.md "Output formats: YUV 4:2:0"): coef = yb, yg, yr, cbb, cbg, cbr, crb, crg, crr and the Y offset
void output_yuv_matrix(int id, int coef[9], int* yoff);
// the normalisations rip_set_output_normalization accepts: everything finite, divisor != 0, std_c != 0; throws std::invalid_argument
void check_output_normalization(double divisor, const double mean[3], const double sd[3]);
// The 3 x 256 table of a planar format (ids 3 .. 8), plane-major, in the format's element type: for plane c and value v,
// y = (v / divisor - mean_c) / std_c in double, every operation rounded, T_c[v] = (float)y; f16 / bf16 entries are that float
// rounded to nearest even (overflow to +-inf and subnormals as IEEE 754 says).  out: 768 elements of 4 / 2 / 2 bytes.
void build_output_table(int format, double divisor, const double mean[3], const double sd[3], void* out);
// the target sizes rip_set_output_size accepts: (0, 0), or both in 1 .. 16384; throws std::invalid_argument naming the rule
void check_output_size(int width, int height);
// The tables of the resize stage (rip_resize.hip; cv::resize(8U, INTER_LINEAR), imgproc/resize.cpp, as oracle/rip_oracle.c restates
// it) from an R x C image to H x W, every side in 1 .. 16384 (std::invalid_argument otherwise).  Per output column x:
// f = (float)((x + 0.5) * ((double)C / W) - 0.5), sx = floor(f), f -= sx in float; sx < 0: sx = 0, f = 0; sx >= C - 1: sx = C - 1,
// f = 0; xofs[x] = sx, alpha[2x] = cvRound((1.f - f) * 2048), alpha[2x + 1] = cvRound(f * 2048) (half to even).  Per output row y the
// same from R / H without the reset of f: beta[2y], beta[2y + 1], and yofs[2y], yofs[2y + 1] = sy, sy + 1 clamped to [0, R - 1].
// *area2 = 1 when R == 2 H and C == 2 W (OpenCV's switch to the 2 x 2 mean; the tables are filled in all the same).
// xofs: W, alpha: 2 W, yofs: 2 H, beta: 2 H entries.
void build_resize_tables(int R, int C, int H, int W, int32_t* xofs, int16_t* alpha, int32_t* yofs, int16_t* beta, int* area2);
// the same tables without the checks, for sizes of any positive int: the ccc estimator's resize to 360 x 270 of frames with a side
// past 16384 takes them from here
void fill_resize_tables(int R, int C, int H, int W, int32_t* xofs, int16_t* alpha, int32_t* yofs, int16_t* beta);
// the names rip_set_output_interpolation accepts: 0 for "linear", 1 for "area", 2 for "linear_aa", 3 for "cubic_aa"; throws
// std::invalid_argument naming them otherwise
int output_interpolation_id(const std::string& name);
// The sizes the area interpolation takes, from R x C to H x W: every side in 1 .. 16384, no upscale (H <= R, W <= C) and a factor of at
// most 256 per axis (R <= 256 H, C <= 256 W: a block sum stays below 2^24).  Throws std::invalid_argument naming the rule.
void check_resize_area_sizes(int R, int C, int H, int W);
// The sizes the antialiased filters take, from R x C to H x W: every side in 1 .. 16384 and a factor of at most 64 per axis (R <= 64 H,
// C <= 64 W: the source rows one output row reads fit the kernel's LDS); upscales are accepted.  Throws std::invalid_argument.
void check_resize_aa_sizes(int R, int C, int H, int W);
// The tap list of one axis of an antialiased filter (`filter`: 2 = linear_aa, 3 = cubic_aa as output_interpolation_id numbers them;
// PARITY.md "Resize: antialiased filters", every step in double) from s source to d target samples: output i reads the count[i] >= 1
// consecutive source samples from first[i] on, all inside [0, s), with the int16 weights round(w * 2^*prec) that follow each other
// in `weights` in output order; wofs[i] (optional) is where those of output i start.  Returns the number of weights, at most
// resize_aa_weight_capacity(filter, s, d) = 2 S max(s, d) + d with S the filter's support (1 or 2).
size_t resize_aa_weight_capacity(int filter, int s, int d);
size_t build_aa_axis(int filter, int s, int d, int32_t* first, int32_t* count, int32_t* wofs, int16_t* weights, int* prec);
// The tile height of the kernel (rip_aa.hpp) for the vertical axis from s to d rows: the largest of 8, 4, 2, 1 at which the source
// rows any tile's output rows read -- *lds_rows, the largest such span -- times 64 columns times `channels` bytes fit 64 KiB.  A
// height of 1 always fits under the factor cap.  s == d: the pass is skipped and a tile reads its own rows.
int aa_tile_rows(int s, int d, const int32_t* first, const int32_t* count, int channels, int* lds_rows);
// the largest span of source rows a tile of `th` output rows reads
int aa_lds_rows(int s, int d, const int32_t* first, const int32_t* count, int th);
// Both axes from R x C to H x W (check_resize_aa_sizes; std::invalid_argument for a null table or another filter); tile_rows[k] /
// lds_rows[k]: aa_tile_rows for 1 (k = 0) and 3 (k = 1) channels.  xwofs, ywofs, the precisions and the last two may be null.
void build_resize_aa_tables(int filter, int R, int C, int H, int W, int32_t* xfirst, int32_t* xcount, int32_t* xwofs, int16_t* xweight, int* xprec,
                            int32_t* yfirst, int32_t* ycount, int32_t* ywofs, int16_t* yweight, int* yprec, int tile_rows[2], int lds_rows[2]);
// the windows rip_set_output_roi accepts: (0, 0, 0, 0), or x, y >= 0 with width and height in 1 .. 16384; throws std::invalid_argument
void check_output_roi(int x, int y, int width, int height);
// the names rip_set_output_fit accepts: 0 for "stretch", 1 for "letterbox", 2 for "crop"; throws std::invalid_argument naming them otherwise
int output_fit_id(const std::string& name);
// the pad colours rip_set_output_pad accepts: every component in 0 .. 255; throws std::invalid_argument
void check_output_pad(int b, int g, int r);
// the pad byte of a one-channel result: the grey value (3735 b + 19235 g + 9798 r + 16384) >> 15 of the colour, as "mono8" computes it
int output_pad_grey(int b, int g, int r);
// The geometry of the resize stage with a window and a fit mode (PARITY.md "Resize: window and fit"; integers, C division), for a
// final image F of R x C: roi = (x, y, w, h) or four zeros for all of F; (W, H) the target or (0, 0) for none; fit as
// output_fit_id numbers it.  src_xywh: the rectangle of F that is read (the window, shrunk to the target's aspect under "crop");
// dst_xywh: the rectangle of the delivered image that holds picture (all of it except under "letterbox"); the delivered image is
// H x W, or the window's size without a target.  Throws std::invalid_argument for a window that does not lie inside F.
void output_window_geometry(int C, int R, const int roi[4], int W, int H, int fit, int src_xywh[4], int dst_xywh[4]);
// The tap list of one axis of the area interpolation (cv::resize(8U, INTER_AREA), imgproc/resize.cpp computeResizeAreaTab, in double;
// PARITY.md "Resize: area interpolation") from s source to d target samples, d <= s: output i reads the count[i] >= 1 consecutive
// source samples from first[i] on, all inside [0, s), with the float weights that follow each other in `weights` in output order
// (those of output i start at the sum of count[0 .. i)).  Returns the number of weights, at most s + 2 d.
size_t build_area_axis(int s, int d, int32_t* first, int32_t* count, float* weights);
// Both axes of the area interpolation from R x C to H x W (check_resize_area_sizes; std::invalid_argument for a null table):
// xfirst / xcount [W] and xweight [up to C + 2 W], yfirst / ycount [H] and yweight [up to R + 2 H].  *whole = 1 when R % H == 0 and
// C % W == 0 other than the identity and the 2 x 2 mean: the kernel then sums ky x kx blocks and multiplies by *scale =
// 1.f / (float)(ky * kx); else *scale = 0.  The tables are filled in all the same.  whole and scale may be null.
void build_resize_area_tables(int R, int C, int H, int W, int32_t* xfirst, int32_t* xcount, float* xweight, int32_t* yfirst, int32_t* ycount,
                              float* yweight, int* whole, float* scale);
bool load_camera_calibration_file(Modules& m, const std::string& path); // undistortion.cpp:157-195
bool load_color_calibration_file(Modules& m, const std::string& path);  // color_calibration.cpp:52-76
void apply_example_camera_calibration(Modules& m);  // values of config/alphasense_calib_example.yaml
void apply_example_color_calibration(Modules& m);   // values of config/alphasense_color_calib_example.yaml

// ---------------------------------------------------------------------------------------------
// Constant tables
// ---------------------------------------------------------------------------------------------
// gamma_correction.cpp:35-43
void build_gamma_lut(double k, uint8_t lut[256]);

// 8-bit Lab (OpenCV 4.2 imgproc/color_lab.cpp initLabTabs, RGB2Lab_b, Lab2RGBinteger) and
// 8-bit HSV (color_hsv.cpp RGB2HSV_b) tables.
struct ColorTables {
  uint16_t srgb_gamma[256];   // sRGBGammaTab_b
  uint16_t cbrt[3072];        // LabCbrtTab_b
  uint16_t lab_to_yf[512];    // LabToYF_b: {y, ify} pairs
  uint16_t inv_gamma[4096];   // sRGBInvGammaTab_b
  int32_t fwd[9];             // BGR -> XYZ/white, Q12, memory order B,G,R per row
  int32_t inv[9];             // XYZ -> B,G,R rows, Q12
  int32_t sdiv[256], hdiv180[256];
};
const ColorTables& color_tables();  // built once

// vignetting_correction.cpp:32-63: the float mask plane (rows x cols, tightly packed), evaluated with the
// reference's operation order (sqrt, pow(r, 2), pow(r, 4) in double); uploaded once per geometry / parameter set
void build_vignette_mask(int rows, int cols, double scale, double a2, double a4, std::vector<float>& mask, int fp_contract = 0);

// ---------------------------------------------------------------------------------------------
// Debug stage dumps (raw_image_pipeline.hpp:179-186 saveDebugImage): cv::normalize(NORM_MINMAX, 0..255) over all
// channels of the 8-bit image, then cv::imwrite to a .png
// ---------------------------------------------------------------------------------------------
// scale = 255 / (max - min) (0 when max == min), shift = -min * scale in double; per byte
// saturate_cast<uchar>(v * (float)scale + (float)shift), float multiply then add, round half to even (convertTo 8U -> 8U)
void normalize_minmax_u8(uint8_t* data, size_t n);
// 8-bit PNG, grey (channels 1) or colour (channels 3, BGR in memory -> RGB in the file, as cv::imwrite does); the zlib
// stream uses stored blocks (no compression: a debugging aid, not an encoder).  false when the file cannot be written.
bool write_png(const std::string& path, const uint8_t* data, int rows, int cols, int channels);

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
