// rip_plan.cpp -- what one frame geometry / encoding turns into (Plan), the output stage on top of it and the layout of the
// delivered buffer.  Arithmetic and checks on the handle's parameters only: this unit makes no HIP call.
#include "rip_handle.hpp"
#include "rip_unpack.hpp"

namespace rip::api {

int parse_bayer(const std::string& e, int& ry, int& rx) {
  // position of the R sample in the 2x2 cell for the ROS pattern names (debayer.cpp:48-70)
  if (e == "bayer_rggb8") { ry = 0; rx = 0; return 1; }
  if (e == "bayer_grbg8") { ry = 0; rx = 1; return 1; }
  if (e == "bayer_gbrg8") { ry = 1; rx = 0; return 1; }
  if (e == "bayer_bggr8") { ry = 1; rx = 1; return 1; }
  return 0;
}
bool is_bayer16(const std::string& e) {
  return e == "bayer_bggr16" || e == "bayer_gbrg16" || e == "bayer_grbg16" || e == "bayer_rggb16";
}
// bayer_<pattern><suffix> of the packed 10- / 12-bit formats (rip.h "Packed Bayer frames"): the R sample's phase and the layout
// (rip::PackedLayout), or 0
int parse_packed(const std::string& e, int& ry, int& rx) {
  static const struct { const char* suffix; int layout; } kSuffixes[] = {
      {"10p", rip::PACKED_10P}, {"12p", rip::PACKED_12P}, {"10_csi2", rip::PACKED_10_CSI2}, {"12_csi2", rip::PACKED_12_CSI2}};
  if (e.size() < 13 || e.compare(0, 6, "bayer_") != 0) return 0;
  const std::string suffix = e.substr(10);
  for (const auto& k : kSuffixes)
    if (suffix == k.suffix && parse_bayer(e.substr(0, 10) + "8", ry, rx)) return k.layout;
  return 0;
}

// tightly packed bytes of one delivered frame
size_t delivered_bytes(const Plan& pl) { return (size_t)pl.dl_rows * pl.dl_cols * pl.dl_channels * (size_t)pl.dl_elem_bytes; }

// payload bytes of one input row: ceil(cols * B / 8) for a packed format, cols * channels samples otherwise
size_t row_bytes(const Plan& pl, int cols, int channels) {
  if (pl.packed_layout) return rip::packed_row_bytes(pl.packed_layout, cols);
  return (size_t)cols * (size_t)channels * (size_t)pl.in_elem_bytes;
}

// ------------------------------------------------------------------------------------------------
// planning: raw_image_pipeline.hpp:143-172 stage gating
// ------------------------------------------------------------------------------------------------
Plan make_plan(const rip::Modules& m, int rows, int cols, int channels, const std::string& encoding) {
  Plan pl;
  if (rows < 1 || cols < 1) throw AssertError("empty image");
  // the kernels address one frame with 32-bit byte offsets and 24-bit row multiplies
  if (cols > (1 << 22) || rows > (1 << 22) || (unsigned long long)rows * cols * 3ull >= (1ull << 32))
    throw InvalidArgument("image too large: a frame must stay below 4 GiB and 4 Mpx per side");
  pl.encoding_out = encoding;
  if (parse_bayer(encoding, pl.ry, pl.rx)) {
    if (channels != 1) throw AssertError("cv::demosaicing: Bayer input must have one channel");
    if (rows < 3 || cols < 3) throw AssertError("cv::demosaicing: image too small");
    pl.src_kind = rip::SRC_BAYER;
    pl.channels = 3;
    pl.encoding_out = "bgr8";
  } else if (is_bayer16(encoding)) {
    // debayer.cpp:76-78 throws for these names; rip_set_debayer_16bit(1) opts into the extension instead
    if (!m.debayer_16bit) throw InvalidArgument("Encoding [" + encoding + "] is a valid pattern but is not supported!");
    if (channels != 1) throw AssertError("cv::demosaicing: Bayer input must have one channel");
    if (rows < 3 || cols < 3) throw AssertError("cv::demosaicing: image too small");
    std::string e8 = encoding.substr(0, encoding.size() - 2) + "8";
    parse_bayer(e8, pl.ry, pl.rx);
    pl.src_kind = rip::SRC_BAYER;
    pl.in_elem_bytes = 2;
    pl.channels = 3;
    if (m.raw16_white > 0) {  // narrowed right after the demosaic: an 8-bit frame from there on
      pl.raw16 = true;
      pl.black = m.raw16_black;
      pl.white = m.raw16_white;
      pl.encoding_out = "bgr8";
    } else {
      pl.out_elem_bytes = 2;
      pl.encoding_out = "bgr16";
    }
  } else if (const int layout = parse_packed(encoding, pl.ry, pl.rx)) {
    // no reference behaviour to override: accepted whatever rip_set_debayer_16bit says
    if (channels != 1) throw AssertError("cv::demosaicing: Bayer input must have one channel");
    if (rows < 3 || cols < 3) throw AssertError("cv::demosaicing: image too small");
    const int mult = rip::packed_cols_multiple(layout);
    if (cols % mult != 0)
      throw InvalidArgument("Encoding [" + encoding + "]: the width must be a multiple of " + std::to_string(mult) + " (whole CSI-2 groups of " +
                            std::to_string(mult) + " pixels in " + std::to_string(mult * rip::packed_bits(layout) / 8) + " bytes), got " + std::to_string(cols));
    pl.src_kind = rip::SRC_BAYER;
    pl.channels = 3;
    pl.packed_layout = layout;
    pl.raw16 = true;  // narrowed right after the demosaic, never bgr16
    if (m.raw16_white > 0) {
      pl.black = m.raw16_black;
      pl.white = m.raw16_white;
    } else {  // the format's natural range
      pl.black = 0;
      pl.white = (1 << rip::packed_bits(layout)) - 1;
    }
    pl.encoding_out = "bgr8";
  } else if (encoding == "rgb8") {
    if (channels != 3) throw AssertError("cvtColor(RGB2BGR): rgb8 input must have three channels");
    pl.src_kind = rip::SRC_RGB;  // swapped to BGR; the encoding string stays "rgb8" (debayer.cpp:72-73)
    pl.channels = 3;
  } else if (channels == 3) {
    pl.src_kind = rip::SRC_BGR;
    pl.channels = 3;
  } else if (channels == 1) {
    pl.src_kind = rip::SRC_MONO;
    pl.channels = 1;
  } else {
    throw InvalidArgument("images with " + std::to_string(channels) + " channels are not supported");
  }
  pl.mht = pl.src_kind == rip::SRC_BAYER && m.debayer_method == "mht";
  pl.flip_angle = (m.flip_enabled && (m.flip_angle == 90 || m.flip_angle == 180 || m.flip_angle == 270)) ? m.flip_angle : 0;
  const bool swap = pl.flip_angle == 90 || pl.flip_angle == 270;
  pl.mid_rows = swap ? cols : rows;
  pl.mid_cols = swap ? rows : cols;
  if (m.wb_enabled && pl.channels == 3) {
    const std::string& w = m.wb_method;
    if (w == "gray_world" || w == "grey_world")
      pl.wb_mode = rip::WB_Q8;
    else if (w == "ccc")
      pl.wb_mode = rip::WB_FLOAT;
    else if (w == "pca")
      pl.wb_mode = rip::WB_PCA;
    else if (w == "simple")
      pl.wb_mode = rip::WB_SIMPLE;
    else if (w == "learned")
      throw InvalidArgument("White Balance method [learned] (cv::xphoto::LearningBasedWB, a model compiled into opencv_contrib) is not implemented by the MI355X pipeline; use 'simple', 'gray_world', 'ccc' or 'pca'");
    else
      throw InvalidArgument("White Balance method [" + w + "] not supported. Supported algorithms: 'simple', 'gray_world', 'learned', 'ccc', 'pca'");
  }
  if (m.cc_enabled && pl.channels == 3 && m.cc_available) pl.stage_bits |= rip::ST_CC;
  if (m.gamma_enabled) pl.stage_bits |= rip::ST_GAMMA;
  if (m.vig_enabled) {
    if (pl.channels != 3) throw AssertError("cvtColor(BGR2Lab): vignetting correction needs a 3-channel image");
    pl.stage_bits |= rip::ST_VIG;
  }
  if (m.ce_enabled && pl.channels == 3) pl.stage_bits |= rip::ST_HSV;
  pl.remap = m.und_enabled && m.und_available && m.dist_model != "none";
  if (pl.out_elem_bytes == 2 && (pl.wb_mode != rip::WB_NONE || pl.stage_bits != 0 || pl.remap))
    // every later module of the reference works on 8-bit images (cv::LUT, xphoto white balance, 8-bit Lab / HSV tables)
    // and would assert on CV_16UC3
    throw AssertError("16-bit Bayer frames go through debayer and flip only: disable white balance, colour calibration, gamma, "
                      "vignetting, colour enhancer and undistortion (they are 8-bit stages)");
  pl.out_rows = pl.remap ? m.dist_h : pl.mid_rows;
  pl.out_cols = pl.remap ? m.dist_w : pl.mid_cols;
  return pl;
}

// The output stage on top of a plan (rip_set_output_format): what the frame calls and rip_query_output deliver.  The taps, the
// debug dumps and rip_query_taps stay with make_plan's image.  Throws before anything is enqueued where the format does not apply.
// head: whose settings (rip_set_output_heads); the single-output calls pass the selected one.
namespace {
void apply_format_and_size(const rip::Modules& mods, int head, Plan& pl) {
  const rip::OutputHead& m = mods.heads[head];
  pl.head = head;
  pl.dl_channels = pl.channels;
  pl.dl_elem_bytes = pl.out_elem_bytes;
  // the resize stage (rip_set_output_size) sits between F and the format: the delivered geometry is the target's
  pl.img_rows = pl.out_rows;
  pl.dl_cols = pl.dl_pic_cols = pl.out_cols;
  pl.win_w = pl.pic_w = pl.out_cols;
  pl.win_h = pl.pic_h = pl.out_rows;
  const int fit = rip::output_fit_id(m.out_fit);
  pl.fit_geometry = m.roi_w > 0 || (m.out_w > 0 && fit != 0);
  if (pl.fit_geometry) {
    // a window, or a fit mode that changes what a target means (PARITY.md "Resize: window and fit").  The refusals in their order:
    // a bgr16 result, a window outside F, an F beyond the resize's sides, the filter's own rules on window -> picture.
    if (pl.out_elem_bytes != 1)
      throw InvalidArgument("output roi / fit need an 8-bit pipeline result; this frame gives bgr16 (set a 16-bit range, or the roi (0, 0, 0, 0) and the fit 'stretch')");
    const int roi[4] = {m.roi_x, m.roi_y, m.roi_w, m.roi_h};
    int src[4], dst[4];
    rip::output_window_geometry(pl.out_cols, pl.out_rows, roi, m.out_w, m.out_h, fit, src, dst);
    pl.win_x = src[0], pl.win_y = src[1], pl.win_w = src[2], pl.win_h = src[3];
    pl.pic_x = dst[0], pl.pic_y = dst[1], pl.pic_w = dst[2], pl.pic_h = dst[3];
    pl.dl_cols = pl.dl_pic_cols = m.out_w > 0 ? m.out_w : pl.win_w;
    pl.img_rows = m.out_w > 0 ? m.out_h : pl.win_h;
    if (pl.channels == 1) pl.pad[0] = (uint8_t)rip::output_pad_grey(m.out_pad[0], m.out_pad[1], m.out_pad[2]);
    else for (int i = 0; i < 3; i++) pl.pad[i] = (uint8_t)m.out_pad[i];
    // all of F delivered as it is: today's identity rule, nothing is launched
    if (!(pl.win_is_frame() && pl.pic_is_delivered() && pl.dl_cols == pl.out_cols && pl.img_rows == pl.out_rows)) {
      if (pl.out_rows > rip::kRszMaxSide || pl.out_cols > rip::kRszMaxSide)
        throw InvalidArgument("output size: the pipeline's image of " + std::to_string(pl.out_cols) + " x " + std::to_string(pl.out_rows) +
                              " is larger than the " + std::to_string(rip::kRszMaxSide) + " pixels per side the resize takes");
      // a picture of the window's own size is a copy, which the linear tables are (weights 2048 and 0) under either interpolation
      const int filter = rip::output_interpolation_id(m.out_interp);
      if (filter == 1 && !(pl.win_w == pl.pic_w && pl.win_h == pl.pic_h)) {
        rip::check_resize_area_sizes(pl.win_h, pl.win_w, pl.pic_h, pl.pic_w);
        pl.rsz_kind = pl.win_h == 2 * pl.pic_h && pl.win_w == 2 * pl.pic_w ? 0 : 1;
      } else if (filter >= 2 && !(pl.win_w == pl.pic_w && pl.win_h == pl.pic_h)) {
        // the antialiased filters' own refusal (a factor beyond 64); no 2 x 2 special case under these names
        rip::check_resize_aa_sizes(pl.win_h, pl.win_w, pl.pic_h, pl.pic_w);
        pl.rsz_kind = filter;
      }
      pl.rsz_active = true;
    }
  } else if (m.out_w > 0) {
    if (pl.out_elem_bytes != 1)
      throw InvalidArgument("output size (" + std::to_string(m.out_w) + ", " + std::to_string(m.out_h) +
                            ") needs an 8-bit pipeline result; this frame gives bgr16 (set a 16-bit range, or the output size (0, 0))");
    if (m.out_w != pl.out_cols || m.out_h != pl.out_rows) {
      if (pl.out_rows > rip::kRszMaxSide || pl.out_cols > rip::kRszMaxSide)
        throw InvalidArgument("output size: the pipeline's image of " + std::to_string(pl.out_cols) + " x " + std::to_string(pl.out_rows) +
                              " is larger than the " + std::to_string(rip::kRszMaxSide) + " pixels per side the resize takes");
      const int filter = rip::output_interpolation_id(m.out_interp);
      if (filter == 1) {
        // the area interpolation's own refusals (an upscale, a factor beyond 256); the exact 2 x 2 case is the linear path's mean
        rip::check_resize_area_sizes(pl.out_rows, pl.out_cols, m.out_h, m.out_w);
        pl.rsz_kind = pl.out_rows == 2 * m.out_h && pl.out_cols == 2 * m.out_w ? 0 : 1;
      } else if (filter >= 2) {
        rip::check_resize_aa_sizes(pl.out_rows, pl.out_cols, m.out_h, m.out_w);  // a factor beyond 64
        pl.rsz_kind = filter;
      }
      pl.rsz_active = true;
      pl.img_rows = m.out_h;
      pl.dl_cols = m.out_w;
      pl.pic_w = pl.dl_cols;
      pl.pic_h = pl.img_rows;
    }
  }
  pl.dl_rows = pl.img_rows;
  pl.dl_pic_cols = pl.dl_cols;
  const int fmt = rip::output_format_id(m.out_format);
  if (fmt == rip::OUT_NATIVE) return;
  pl.fmt_active = true;
  if (pl.out_elem_bytes != 1)
    throw InvalidArgument("output format [" + m.out_format + "] needs an 8-bit pipeline result; this frame gives bgr16 (set a 16-bit range, or the format 'native')");
  if (rip::output_format_jpeg(fmt)) {
    // One slot per frame: a one-channel row of the default slot's bytes; img_rows x dl_pic_cols stays the picture that is coded, one
    // component from a one-channel result, Y Cb Cr 4:2:0 from B, G, R (PARITY.md "Output formats: JPEG").  The refusals: CLAHE on the
    // head, then what the stream's 16-bit fields cannot hold.
    if (m.clahe_tiles_x != 0)
      throw InvalidArgument("output format [jpeg] does not take CLAHE on the same head (set the clahe tiles (0, 0), or another format)");
    if (pl.dl_cols > 65535 || pl.img_rows > 65535)
      throw InvalidArgument("output format [jpeg]: a delivered picture of " + std::to_string(pl.dl_cols) + " x " + std::to_string(pl.img_rows) + " is beyond the 65535 pixels per side a JPEG frame header holds");
    if ((long long)m.jpeg_restart_rows * rip::jpeg_mcus_x(pl.dl_cols, pl.channels) > 65535)
      throw InvalidArgument("output format [jpeg]: " + std::to_string(m.jpeg_restart_rows) + " MCU rows of " + std::to_string(rip::jpeg_mcus_x(pl.dl_cols, pl.channels)) +
                            " MCUs are beyond the 65535 MCUs a restart interval holds (set fewer restart rows)");
    pl.jpeg_quality = m.jpeg_quality;
    pl.jpeg_restart_rows = m.jpeg_restart_rows;
    pl.out_fmt = fmt;
    pl.dl_channels = 1;
    pl.dl_elem_bytes = 1;
    pl.dl_rows = 1;
    const size_t slot = rip::jpeg_default_slot(pl.img_rows, pl.dl_pic_cols, pl.channels, m.jpeg_restart_rows);
    if (slot > 0x7FFFFFFFull) throw InvalidArgument("output format [jpeg]: the default slot of " + std::to_string(slot) + " bytes is beyond 2 GiB");
    pl.dl_cols = (int)slot;
    pl.encoding_out = m.out_format;
    return;
  }
  if (pl.channels == 1) {
    if (fmt != rip::OUT_MONO8)
      throw InvalidArgument("output format [" + m.out_format + "] needs a three-channel pipeline result; this frame gives one channel ('mono8' and 'native' apply)");
    pl.encoding_out = "mono8";  // the identity: no kernel
    return;
  }
  if (rip::output_format_yuv(fmt)) {
    // 4:2:0 has one chroma sample per 2 x 2 block of the delivered picture.  The delivered buffer is the one-channel image of 3 H / 2
    // rows x W bytes that holds the three planes; img_rows stays the picture's H (PARITY.md "Output formats: YUV 4:2:0")
    if ((pl.dl_cols | pl.img_rows) & 1)
      throw InvalidArgument("output format [" + m.out_format + "] needs a delivered picture of even width and height (one chroma sample per 2 x 2 block); this one is " +
                            std::to_string(pl.dl_cols) + " x " + std::to_string(pl.img_rows));
    pl.dl_rows = pl.img_rows / 2 * 3;
    pl.yuv_matrix = rip::output_yuv_matrix_id(m.out_yuv_matrix);
  }
  pl.out_fmt = fmt;
  pl.dl_channels = rip::output_format_channels(fmt);
  pl.dl_elem_bytes = rip::output_format_elem_bytes(fmt);
  pl.dl_planar = rip::output_format_planar(fmt);
  pl.encoding_out = m.out_format;
}
}  // namespace

// The format, the resize and -- behind every refusal of theirs -- CLAHE on the delivered one-channel picture (rip_set_output_clahe;
// PARITY.md "Local contrast: CLAHE"), which changes nothing about the delivered geometry.
void apply_output_format(const rip::Modules& mods, int head, Plan& pl) {
  apply_format_and_size(mods, head, pl);
  const rip::OutputHead& m = mods.heads[head];
  if (m.clahe_tiles_x == 0 || rip::output_format_jpeg(pl.out_fmt)) return;
  if (pl.dl_channels != 1 || pl.dl_elem_bytes != 1 || rip::output_format_yuv(pl.out_fmt))
    throw InvalidArgument("output clahe needs a delivered one-channel 8-bit picture; this head delivers [" + pl.encoding_out + "] (set the output format 'mono8', or the clahe tiles (0, 0))");
  if (pl.pic_w < 2 * m.clahe_tiles_x || pl.pic_h < 2 * m.clahe_tiles_y)
    throw InvalidArgument("output clahe: the delivered picture of " + std::to_string(pl.pic_w) + " x " + std::to_string(pl.pic_h) + " is smaller than two pixels per tile and side under the tiles (" +
                          std::to_string(m.clahe_tiles_x) + ", " + std::to_string(m.clahe_tiles_y) + ")");
  pl.clahe = true;
  pl.clahe_tx = m.clahe_tiles_x;
  pl.clahe_ty = m.clahe_tiles_y;
  pl.clahe_clip = m.clahe_clip_limit;
}

// The tightly packed DELIVERED frames at d_out: what a row pitch and a frame stride of 0 stand for.  Planar formats: `step` is
// the row pitch inside a plane and a frame is three planes of step * rows.
FrameView tight_output_view(const Plan& pl, void* d_out) {
  const size_t step = (size_t)pl.dl_cols * (size_t)pl.dl_elem_bytes * (pl.dl_planar ? 1 : (size_t)pl.dl_channels);
  return {static_cast<uint8_t*>(d_out), step, step * (size_t)pl.dl_rows * (pl.dl_planar ? 3 : 1), pl.dl_rows, pl.dl_cols};
}

// The delivered frames of rip_apply_device (0 = tight), with the checks rip.h promises.  The kernels address one frame with
// 32-bit byte offsets and 24-bit row multiplies: pitches they cannot express, and pitches that would make rows or frames
// overlap, are refused instead of writing somewhere else.
FrameView resolve_output_layout(const Plan& pl, void* d_out, size_t out_step, size_t out_frame_stride) {
  FrameView v = tight_output_view(pl, d_out);
  if (rip::output_format_jpeg(pl.out_fmt)) {
    // a row pitch is the capacity of a slot: any the header and EOI fit in; the streams are written at any alignment
    const size_t least = (size_t)rip::jpeg_header_bytes(pl.channels) + 2;
    if (out_step) v.step = out_step;
    if (v.step < least) throw InvalidArgument("output format [jpeg]: a slot of " + std::to_string(v.step) + " bytes is smaller than the header and EOI (" + std::to_string(least) + " bytes)");
    if (v.step > 0xFFFFFFFFull) throw InvalidArgument("output format [jpeg]: a slot must stay below 4 GiB");
    v.frame_stride = out_frame_stride ? out_frame_stride : v.step;
    if (v.frame_stride < v.step) throw InvalidArgument("output frame stride smaller than a frame");
    return v;
  }
  const size_t e = (size_t)pl.dl_elem_bytes, row = v.step;
  if (out_step) v.step = out_step;
  if (v.step < row) throw InvalidArgument("output row pitch smaller than a row");
  // i420: the chroma rows are half a pitch apart
  if (pl.out_fmt == rip::OUT_I420 && (v.step & 1)) throw InvalidArgument("output format [i420] needs an even row pitch (a chroma row is half of it), got " + std::to_string(v.step));
  const unsigned long long frame = (unsigned long long)v.step * pl.dl_rows * (pl.dl_planar ? 3ull : 1ull);
  v.frame_stride = out_frame_stride ? out_frame_stride : (size_t)frame;
  if (v.frame_stride < frame) throw InvalidArgument("output frame stride smaller than a frame");
  if (v.step >= (1u << 24) || frame >= (1ull << 32)) throw InvalidArgument("row pitch too large: pitches must stay below 16 MiB and a frame below 4 GiB");
  // native results are bytes, or bgr16 samples whose alignment has never been asked for
  if (pl.out_fmt != rip::OUT_NATIVE && (reinterpret_cast<uintptr_t>(d_out) | v.step | v.frame_stride) % e != 0)
    throw InvalidArgument("output buffer, row pitch and frame stride must be multiples of the element size (" + std::to_string(e) + " bytes)");
  return v;
}

// The caller's frames of rip_apply_device and rip_apply_device_heads (0 = tight) under the same limits as the output: 32-bit byte
// offsets inside a frame, 24-bit row multiplies.  The refusals come in two steps, so that rip_apply_device can place refusals of its
// own between them: resolve_input_pitches is the first, and running it again on resolved pitches changes nothing.
void resolve_input_pitches(const Plan& pl, int rows, int cols, int channels, size_t& in_step, size_t& in_frame_stride) {
  const size_t in_row = row_bytes(pl, cols, channels);
  if (in_step == 0) in_step = in_row;
  if (in_frame_stride == 0) in_frame_stride = in_step * rows;
  if (in_step < in_row) throw InvalidArgument("input row pitch smaller than a row");
}

ConstFrameView resolve_input_layout(const Plan& pl, const void* d_in, size_t in_step, size_t in_frame_stride, int rows, int cols, int channels) {
  resolve_input_pitches(pl, rows, cols, channels, in_step, in_frame_stride);
  if (in_frame_stride < in_step * (size_t)(rows - 1) + row_bytes(pl, cols, channels)) throw InvalidArgument("input frame stride smaller than a frame");
  if (in_step >= (1u << 24) || (unsigned long long)in_step * rows >= (1ull << 32))
    throw InvalidArgument("row pitch too large: pitches must stay below 16 MiB and a frame below 4 GiB");
  return {static_cast<const uint8_t*>(d_in), in_step, in_frame_stride, rows, cols};
}

}  // namespace rip::api
