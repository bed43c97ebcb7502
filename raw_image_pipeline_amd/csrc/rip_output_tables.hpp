// rip_output_tables.hpp -- the host-built tables and geometry of the output stage: the planar formats' 3 x 256 table, the YUV
// matrices, the window geometry, and the tables of the three resize filters with their size checks.  The unit stands on its own:
// the host-side kernel tests link rip_output_tables.cpp and nothing else of the library.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rip {

// the integers of matrix `id` (PARITY.md "Output formats: YUV 4:2:0"): coef = yb, yg, yr, cbb, cbg, cbr, crb, crg, crr and the Y offset
void output_yuv_matrix(int id, int coef[9], int* yoff);
// the normalisations rip_set_output_normalization accepts: everything finite, divisor != 0, std_c != 0; throws std::invalid_argument
void check_output_normalization(double divisor, const double mean[3], const double sd[3]);
// The 3 x 256 table of a planar format (ids 3 .. 8), plane-major, in the format's element type: for plane c and value v,
// y = (v / divisor - mean_c) / std_c in double, every operation rounded, T_c[v] = (float)y; f16 / bf16 entries are that float
// rounded to nearest even (overflow to +-inf and subnormals as IEEE 754 says).  out: 768 elements of 4 / 2 / 2 bytes.
void build_output_table(int format, double divisor, const double mean[3], const double sd[3], void* out);
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

}  // namespace rip
