// rip_output_stage.cpp -- everything behind the pipeline's image F: the staging image the chain's last kernel writes, the resize,
// pad, converter and YUV launches of one output head (prepare_head, enqueue_head), several heads from one run of the chain
// (run_batch_heads) and the valid-pixel masks, which run a head's launches on the coverage image.  The kernels live in the
// kernel libraries (rip_output/resize/area/fit/aa/heads/mask/yuv/clahe/jpeg.hpp; CLAHE's two launches end a head that equalises its
// picture); the chain in front is rip_batch.cpp's run_batch.
#include <algorithm>

#include "rip_handle.hpp"

namespace rip::api {

// pitch of the staging image in front of the resize and the converter: every source row starts 16-byte aligned
size_t fmt_pitch(const Plan& pl) { return pitch16((size_t)pl.out_cols * pl.channels); }

namespace {

// where a launch behind F reads and writes: the three source and the three destination fields of the libraries' parameter blocks
template <typename P>
void bind_src(P& d, ConstFrameView v) {
  d.src = v.ptr;
  d.src_step = v.step;
  d.src_frame_stride = v.frame_stride;
}
template <typename P>
void bind_dst(P& d, const FrameView& v) {
  d.dst = v.ptr;
  d.dst_step = v.step;
  d.dst_frame_stride = v.frame_stride;
}

// The fields ResizeParams, AreaParams and AaParams (P) have in common, bound into the block `r` that already holds the head's tables:
// the window of F in `staged` that is read -- its size; its origin goes to the launch -- and the picture's rectangle `to` of F' that
// is written, for n frames.
template <typename P>
P resize_params(P r, const FrameView& staged, const FrameView& to, const Plan& pl, int n) {
  bind_src(r, staged);
  bind_dst(r, to);
  r.src_rows = pl.win_h;
  r.src_cols = pl.win_w;
  r.rows = pl.pic_h;
  r.cols = pl.pic_w;
  r.channels = pl.channels;
  r.n_frames = n;
  return r;
}

// the staging image F of a plan, not yet allocated: 16-byte aligned pitch and frame stride
FrameView staging_view(const Plan& pl) { return {nullptr, fmt_pitch(pl), fmt_pitch(pl) * (size_t)pl.out_rows, pl.out_rows, pl.out_cols}; }

// F' in front of the converter (only under a resize and a format), not yet allocated: the converter's source alignment
FrameView resized_view(const Plan& pl) {
  const size_t pitch = pitch16((size_t)pl.dl_pic_cols * pl.channels);
  return {nullptr, pitch, pitch * (size_t)pl.img_rows, pl.img_rows, pl.dl_pic_cols};
}

// What one head's launches behind F need besides its plan, made ready before the first launch of the batch (the ensure_* functions
// upload and wait): the parameter block of its resize with the tables in it -- the one of pl.rsz_kind -- and what the converter
// reads -- F, or F' in d_rsz behind a resize
struct HeadPrep {
  FrameView converted_from{};
  rip::ResizeParams linear = {};
  rip::AreaParams area = {};
  rip::AaParams aa = {};
};

// bytes of d_rsz a head needs for n frames: F' in front of the converter, only under a resize and a format
size_t rsz_bytes(const Plan& pl, int n) {
  if (!pl.rsz_active || pl.out_fmt == rip::OUT_NATIVE) return 0;
  return resized_view(pl).frame_stride * (size_t)n;
}

// bytes of d_jpeg_coef / d_jpeg_intervals a head needs for n frames: 0 unless it delivers "jpeg"
size_t jpeg_coef_scratch(const Plan& pl, int n) { return rip::output_format_jpeg(pl.out_fmt) ? rip::jpeg_coef_bytes(pl.img_rows, pl.dl_pic_cols, pl.channels, n) : 0; }
size_t jpeg_interval_scratch(const Plan& pl, int n) {
  return rip::output_format_jpeg(pl.out_fmt) ? rip::jpeg_interval_bytes(pl.img_rows, pl.channels, pl.jpeg_restart_rows, n) : 0;
}

// bytes of d_clahe a head needs for n frames: the tables of its CLAHE
size_t clahe_bytes(const Plan& pl, int n) { return pl.clahe ? rip::clahe_lut_bytes(pl.clahe_tx, pl.clahe_ty, n) : 0; }

// the scratch of the handle a head's launches use for n frames: bytes of d_rsz, d_clahe, d_jpeg_coef and d_jpeg_intervals
struct HeadScratch {
  size_t rsz, clahe, jpeg_coef, jpeg_intervals;
};
HeadScratch head_scratch(const Plan& pl, int n) { return {rsz_bytes(pl, n), clahe_bytes(pl, n), jpeg_coef_scratch(pl, n), jpeg_interval_scratch(pl, n)}; }
HeadScratch max(const HeadScratch& a, const HeadScratch& b) {
  return {std::max(a.rsz, b.rsz), std::max(a.clahe, b.clahe), std::max(a.jpeg_coef, b.jpeg_coef), std::max(a.jpeg_intervals, b.jpeg_intervals)};
}
// The heads of a batch run one after another and share the scratch: reserved for the largest before the first of them is prepared,
// so that a head's own reserve finds room and no buffer moves once a HeadPrep points into it.
void reserve_head_scratch(rip_pipeline* p, const HeadScratch& s) {
  p->d_rsz.reserve(s.rsz);
  p->d_clahe.reserve(s.clahe);
  p->d_jpeg_coef.reserve(s.jpeg_coef);
  p->d_jpeg_intervals.reserve(s.jpeg_intervals);
}

HeadPrep prepare_head(rip_pipeline* p, const Plan& pl, const FrameView& staged, int n) {
  HeadPrep hp;
  reserve_head_scratch(p, head_scratch(pl, n));
  if (pl.dl_planar) ensure_output_table(p, pl.head, pl.out_fmt);
  hp.converted_from = staged;  // what the converter reads: F, or F' behind a resize
  if (pl.rsz_active) {
    // from the window that is read to the picture that is written: all of F and all of F' unless a window or a fit mode is set
    if (pl.rsz_kind >= 2) ensure_aa_tables(p, pl.head, pl.rsz_kind, pl.channels, pl.win_h, pl.win_w, pl.pic_h, pl.pic_w, hp.aa);
    else if (pl.rsz_kind == 1) ensure_area_tables(p, pl.head, pl.win_h, pl.win_w, pl.pic_h, pl.pic_w, hp.area);
    else ensure_resize_tables(p, pl.head, pl.win_h, pl.win_w, pl.pic_h, pl.pic_w, hp.linear);
    if (pl.out_fmt != rip::OUT_NATIVE) {
      hp.converted_from = resized_view(pl);
      hp.converted_from.ptr = p->d_rsz.as<uint8_t>();
    }
  }
  if (rip::output_format_jpeg(pl.out_fmt)) ensure_jpeg_constants(p, pl);
  return hp;
}

// every launch behind F: a refusal is a bug of the frame call's checks; then the launch error, then the launch record
void launched(bool accepted, const rip::LaunchInfo& info, const char* what, int n) {
  if (!accepted) throw DeviceError(std::string("internal: ") + what + " refused a layout the frame call had accepted");
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) throw DeviceError(std::string("kernel launch failed: ") + hipGetErrorString(le));
  RIP_LOG_LAUNCH(dim3(info.grid_x, info.grid_y), info.block, n, "%s", info.kernel);
}

// The launches behind F for one head up to its delivered image: the resize, window resize, area or antialiased launch, then the pad,
// then the converter, reading F in `staged` (16-byte aligned base, pitch and frame stride) and writing the head's delivered frames `dst`.
// first_frame: the index, inside the frame call, of the slice's first frame -- where a jpeg head's stream lengths go.
void enqueue_head_image(rip_pipeline* p, const Plan& pl, const HeadPrep& hp, const FrameView& staged, FrameView dst, int n, int first_frame) {
  // F': the caller's buffer under "native", else the second staging image; the picture's rectangle of it is what the resize writes
  const FrameView whole_to = pl.out_fmt != rip::OUT_NATIVE ? hp.converted_from : dst;
  FrameView to = whole_to;
  to.ptr += (size_t)pl.pic_y * to.step + (size_t)pl.pic_x * pl.channels;
  // a window other than F is read in place by the kernels of librip_fit_hip.so, which take the window's origin; no copy of it is made
  const rip::FitWindow win = {pl.win_x, pl.win_y, pl.out_cols, pl.out_rows};
  rip::LaunchInfo info = {};
  if (pl.rsz_active && pl.rsz_kind >= 2) {  // an antialiased filter: one launch function for all of F and for a window
    const rip::AaParams r = resize_params(hp.aa, staged, to, pl, n);
    launched(rip::launch_aa(r, win, p->stream, &info), info, "the antialiased resize", n);
  } else if (pl.rsz_active && pl.rsz_kind == 1) {
    const rip::AreaParams r = resize_params(hp.area, staged, to, pl, n);
    if (!pl.win_is_frame()) launched(rip::launch_fit_area(r, win, p->stream, &info), info, "the area resize of a window", n);
    else launched(rip::launch_area_reduce(r, p->stream, &info), info, "the area resize", n);
  } else if (pl.rsz_active) {
    const rip::ResizeParams r = resize_params(hp.linear, staged, to, pl, n);
    if (!pl.win_is_frame()) launched(rip::launch_fit_resize(r, win, p->stream, &info), info, "the resize of a window", n);
    else launched(rip::launch_resize(r, p->stream, &info), info, "the resize", n);
  }
  if (pl.rsz_active && !pl.pic_is_delivered()) {  // a letterbox: the bands around the picture get the pad colour
    rip::FitPadParams f = {};
    bind_dst(f, whole_to);
    f.rows = pl.img_rows;
    f.cols = pl.dl_pic_cols;
    f.pic_x = pl.pic_x;
    f.pic_y = pl.pic_y;
    f.pic_w = pl.pic_w;
    f.pic_h = pl.pic_h;
    f.channels = pl.channels;
    f.n_frames = n;
    for (int i = 0; i < 4; i++) f.color[i] = pl.pad[i];
    launched(rip::launch_fit_pad(f, p->stream, &info), info, "the letterbox pad", n);
  }
  if (pl.out_fmt == rip::OUT_NATIVE) return;
  if (rip::output_format_jpeg(pl.out_fmt)) {  // librip_jpeg_hip.so's four kernels in the converter's place, from the same source
    rip::JpegParams c = {};
    bind_src(c, hp.converted_from);
    bind_dst(c, dst);  // dst.step: the capacity of a slot
    c.rows = pl.img_rows;
    c.cols = pl.dl_pic_cols;
    c.channels = pl.channels;
    c.n_frames = n;
    c.restart_rows = pl.jpeg_restart_rows;
    int coef[9];
    rip::output_yuv_matrix(rip::output_yuv_matrix_id("bt601_full"), coef, &c.m.yoff);  // JFIF: full-range BT.601, whatever the head's matrix
    for (int i = 0; i < 3; i++) c.m.y[i] = coef[i], c.m.cb[i] = coef[3 + i], c.m.cr[i] = coef[6 + i];
    c.tables = p->d_jpeg_tables[pl.head].as<rip::JpegTables>();
    c.header = p->d_jpeg_header[pl.head].as<uint8_t>();
    c.coef = p->d_jpeg_coef.as<int16_t>();
    c.intervals = p->d_jpeg_intervals.as<uint32_t>();
    if (p->jpeg_frames[pl.head] < first_frame + n || p->d_jpeg_sizes[pl.head].cap < (size_t)(first_frame + n) * 4)
      throw DeviceError("internal: the jpeg sizes of the frame call were not reserved");
    c.sizes = p->d_jpeg_sizes[pl.head].as<uint32_t>() + first_frame;
    launched(rip::launch_jpeg_transform(c, p->stream, &info), info, "the JPEG transform", n);
    launched(rip::launch_jpeg_size(c, p->stream, &info), info, "the JPEG sizing pass", n);
    launched(rip::launch_jpeg_scan(c, p->stream, &info), info, "the JPEG scan", n);
    launched(rip::launch_jpeg_write(c, p->stream, &info), info, "the JPEG writing pass", n);
    return;
  }
  if (rip::output_format_yuv(pl.out_fmt)) {  // librip_yuv_hip.so's kernel in the converter's place, from the same source
    rip::Yuv420Params c = {};
    bind_src(c, hp.converted_from);
    bind_dst(c, dst);
    c.rows = pl.img_rows;
    c.cols = pl.dl_cols;
    c.n_frames = n;
    c.semi_planar = pl.out_fmt == rip::OUT_NV12 ? 1 : 0;
    int coef[9];
    rip::output_yuv_matrix(pl.yuv_matrix, coef, &c.m.yoff);
    for (int i = 0; i < 3; i++) c.m.y[i] = coef[i], c.m.cb[i] = coef[3 + i], c.m.cr[i] = coef[6 + i];
    launched(rip::launch_yuv420(c, p->stream, &info), info, "the YUV 4:2:0 converter", n);
    return;
  }
  rip::OutputConvertParams c = {};
  bind_src(c, hp.converted_from);
  bind_dst(c, dst);
  c.rows = pl.img_rows;
  c.cols = pl.dl_cols;
  c.n_frames = n;
  c.format = pl.out_fmt;
  c.table = pl.dl_planar ? p->out_table[pl.head].dev.ptr : nullptr;
  launched(rip::launch_output_convert(c, p->stream, &info), info, "the output converter", n);
}

// Every launch of one head: its delivered image, then CLAHE on the picture's rectangle of it (PARITY.md "Local contrast: CLAHE") -- in
// place in the delivered buffer, or, where nothing else is launched, from the staging image into the delivered buffer.  The tables
// in d_clahe are written by the first launch and read by the second.
void enqueue_head(rip_pipeline* p, const Plan& pl, const HeadPrep& hp, const FrameView& staged, FrameView dst, int n, int first_frame) {
  LaunchLogScope log_scope(p);
  enqueue_head_image(p, pl, hp, staged, dst, n, first_frame);
  if (!pl.clahe) return;
  const bool from_staging = pl.out_fmt == rip::OUT_NATIVE && !pl.rsz_active;
  rip::ClaheParams c = {};
  bind_dst(c, dst);
  c.dst += (size_t)pl.pic_y * dst.step + (size_t)pl.pic_x;
  if (from_staging) bind_src(c, staged);  // the picture is all of F
  else c.src = c.dst, c.src_step = c.dst_step, c.src_frame_stride = c.dst_frame_stride;
  c.lut = p->d_clahe.as<uint8_t>();
  c.rows = pl.pic_h;
  c.cols = pl.pic_w;
  c.n_frames = n;
  rip::clahe_constants(pl.pic_h, pl.pic_w, pl.clahe_tx, pl.clahe_ty, pl.clahe_clip, c);
  rip::LaunchInfo info = {};
  launched(rip::launch_clahe_lut(c, p->stream, &info), info, "the CLAHE tables", n);
  launched(rip::launch_clahe_apply(c, p->stream, &info), info, "the CLAHE blend", n);
}

// a head that launches nothing behind F: the pipeline's image as it is
bool identity_head(const Plan& pl) { return pl.out_fmt == rip::OUT_NATIVE && !pl.rsz_active && !pl.clahe; }

MaskBaseConst::Key mask_base_key(const rip_pipeline* p, bool remap, int src_rows, int src_cols, int rows, int cols) {
  MaskBaseConst::Key k;
  k.generation = remap ? p->maps_generation : 0;  // an all-255 image does not depend on the maps
  k.remap = remap ? 1 : 0;
  k.src_rows = remap ? src_rows : 0;
  k.src_cols = remap ? src_cols : 0;
  k.rows = rows;
  k.cols = cols;
  return k;
}

}  // namespace

// run_batch with the resize and the output stage behind it.  With a target size other than F's, or under a format, the chain's
// last kernel writes the pipeline's image F into the handle's staging buffer; then one launch of the resize (librip_rsz_hip.so, or
// librip_area_hip.so under the area interpolation; librip_fit_hip.so when it reads a window of F, rip_set_output_roi; librip_aa_hip.so
// under an antialiased filter, window or not) writes F' --
// into the caller's buffer under "native", else into a second staging image; under a letterbox it writes the picture's rectangle of
// F' and one launch of the pad kernel fills the rest -- and one launch of the converter (librip_out_hip.so) writes the caller's buffer from F' (or from F without a target).  Neither: this is run_batch.
// dst: the DELIVERED frames.
void run_batch_formatted(rip_pipeline* p, const Plan& pl, ConstFrameView src, FrameView dst, Taps taps, int n, int first_frame) {
  p->head_record[pl.head] = {identity_head(pl) ? 1 : 0, 0};
  if (identity_head(pl)) {
    run_batch(p, pl, src, dst, taps, n);
    return;
  }
  DeviceGuard device_guard(p->device);
  FrameView staged = staging_view(pl);
  p->d_fmt.reserve(staged.frame_stride * (size_t)n);
  staged.ptr = p->d_fmt.as<uint8_t>();
  const HeadPrep hp = prepare_head(p, pl, staged, n);
  run_batch(p, pl, src, staged, taps, n);
  enqueue_head(p, pl, hp, staged, dst, n, first_frame);
}

// Several heads from one run of the chain (rip_apply_device_heads; PARITY.md "Output heads").  One requested head: the function above.
// Else F is written once -- into the first requested identity head whose view is 16-byte aligned in base, pitch and frame stride,
// which then IS the staging image (what d_fmt guarantees by fmt_pitch and hipMalloc, so every launch that reads F takes it; a
// 16-byte block or a dword that holds a byte of a row's end lies inside that byte's page, whatever follows the caller's buffer), else into d_fmt -- and
// every other requested head follows in index order on the handle's stream: one head_copy_kernel launch for an identity head,
// enqueue_head's launches for the others.  d_rsz is shared by the heads, which run one after another: reserved for the largest.
void run_batch_heads(rip_pipeline* p, const Plan& pl, const Plan* plans, const FrameView* dsts, int n_heads, ConstFrameView src, Taps taps, int n, int first_frame) {
  int n_requested = 0, only = -1;
  for (int k = 0; k < n_heads; k++)
    if (dsts[k].ptr) n_requested++, only = k;
  if (n_requested == 1) {
    run_batch_formatted(p, plans[only], src, dsts[only], taps, n, first_frame);
    return;
  }
  DeviceGuard device_guard(p->device);
  int direct = -1;
  for (int k = 0; k < n_heads && direct < 0; k++)
    if (dsts[k].ptr && identity_head(plans[k]) && ((reinterpret_cast<uintptr_t>(dsts[k].ptr) | dsts[k].step | dsts[k].frame_stride) & 15) == 0) direct = k;
  FrameView staged = staging_view(pl);
  if (direct >= 0) {
    staged = dsts[direct];
  } else {
    p->d_fmt.reserve(staged.frame_stride * (size_t)n);
    staged.ptr = p->d_fmt.as<uint8_t>();
  }
  HeadScratch scratch = {};
  for (int k = 0; k < n_heads; k++)
    if (dsts[k].ptr) scratch = max(scratch, head_scratch(plans[k], n));
  reserve_head_scratch(p, scratch);
  HeadPrep hp[rip::kMaxOutputHeads];
  for (int k = 0; k < n_heads; k++)
    if (dsts[k].ptr && !identity_head(plans[k])) hp[k] = prepare_head(p, plans[k], staged, n);
  run_batch(p, pl, src, staged, taps, n);
  for (int k = 0; k < n_heads; k++) {
    if (!dsts[k].ptr) continue;
    p->head_record[k] = {k == direct ? 1 : 0, 0};
    if (k == direct) continue;
    if (!identity_head(plans[k])) {
      enqueue_head(p, plans[k], hp[k], staged, dsts[k], n, first_frame);
      continue;
    }
    LaunchLogScope log_scope(p);
    rip::HeadCopyParams c = {};
    bind_src(c, staged);
    bind_dst(c, dsts[k]);
    c.rows = pl.out_rows;
    c.n_frames = n;
    c.row_bytes = (size_t)pl.out_cols * pl.channels;
    rip::LaunchInfo info = {};
    launched(rip::launch_head_copy(c, p->stream, &info), info, "the head copy", n);
    p->head_record[k].copied = 1;
  }
}

// ---- the format "jpeg": what surrounds the launches (PARITY.md "Output formats: JPEG") ------------------------------------------

void begin_jpeg_call(rip_pipeline* p, const Plan& pl, int n_frames) {
  p->jpeg_frames[pl.head] = 0;  // the lengths of an earlier call are not this call's
  if (!rip::output_format_jpeg(pl.out_fmt)) return;
  DeviceGuard device_guard(p->device);
  p->d_jpeg_sizes[pl.head].reserve((size_t)n_frames * 4);
  p->jpeg_frames[pl.head] = n_frames;
}

void download_jpeg_frame(rip_pipeline* p, const Plan& pl, const void* d_slot, uint8_t* out) {
  uint32_t size = 0;
  HIP_CHECK(hipMemcpyAsync(&size, p->d_jpeg_sizes[pl.head].ptr, 4, hipMemcpyDeviceToHost, p->stream));
  HIP_CHECK(hipStreamSynchronize(p->stream));
  if (size) HIP_CHECK(hipMemcpyAsync(out, d_slot, size, hipMemcpyDeviceToHost, p->stream));
}

// ---- valid-pixel masks (rip_set_rect_mask; PARITY.md "Rect mask") -------------------------------------------------------------

// The mask of a frame geometry (rip_handle.hpp): one launch of rect_mask_kernel (librip_mask_hip.so) over the maps the handle keeps
// on the device, or a fill for a frame that is not undistorted -- its thresholded twin is the same image.
ConstFrameView ensure_mask_base(rip_pipeline* p, bool remap, int src_rows, int src_cols, int rows, int cols, bool binary) {
  DeviceGuard device_guard(p->device);
  LaunchLogScope log_scope(p);
  MaskBaseConst& mb = p->mask_base;
  const MaskBaseConst::Key key = mask_base_key(p, remap, src_rows, src_cols, rows, cols);
  if (!(key == mb.key)) {
    mb.key = key;
    mb.cov_valid = mb.bin_valid = false;
  }
  const bool twin = binary && remap;
  DevBuf& buf = twin ? mb.bin : mb.cov;
  bool& valid = twin ? mb.bin_valid : mb.cov_valid;
  const size_t pitch = mb.pitch();
  if (!valid) {
    p->work_enqueued = true;
    buf.reserve(pitch * (size_t)rows);
    if (remap) {
      ensure_maps(p);
      rip::RectMaskParams r = {};
      r.map_xy = p->maps.dev.as<float>();
      r.drows = rows;
      r.dcols = cols;
      r.src_rows = src_rows;
      r.src_cols = src_cols;
      r.dst = buf.as<uint8_t>();
      r.dst_step = pitch;
      r.binary = binary ? 1 : 0;
      rip::LaunchInfo info = {};
      launched(rip::launch_rect_mask(r, p->stream, &info), info, "the rect mask", 0);
    } else {
      HIP_CHECK(hipMemsetAsync(buf.ptr, 255, pitch * (size_t)rows, p->stream));
    }
    valid = true;
    mb.builds++;
  }
  return {buf.as<uint8_t>(), pitch, pitch * (size_t)rows, rows, cols};
}

// The delivered mask of a head: the head's own launches behind F (prepare_head / enqueue_head) on a copy of the frame's plan that has
// one channel, the format "native" and the pad 0, reading the coverage in place of F; under `valid` the threshold follows the head's
// geometry (mask_threshold_kernel).  A head that delivers F as it is gets a copy of the mask -- under `valid` of its thresholded
// twin, which the kernel wrote directly -- so that every head's image is its own and lives as long as that head's cache.
ConstFrameView ensure_mask_head(rip_pipeline* p, const Plan& frame_pl, int mode) {
  DeviceGuard device_guard(p->device);
  Plan pl = frame_pl;
  pl.channels = pl.dl_channels = 1;
  pl.out_elem_bytes = pl.dl_elem_bytes = 1;
  pl.fmt_active = pl.dl_planar = false;
  pl.clahe = false;  // a mask is coverage, not a picture
  pl.out_fmt = rip::OUT_NATIVE;
  pl.dl_rows = pl.img_rows;  // a mask ignores the format: the picture's rows under a YUV format too
  pl.dl_cols = pl.dl_pic_cols;  // ... and the picture's width under "jpeg", whose delivered row is a slot
  for (uint8_t& c : pl.pad) c = 0;
  const bool identity = identity_head(pl), binary = mode == 2;
  MaskHeadConst& mh = p->mask_head[pl.head];
  const MaskBaseConst::Key key = mask_base_key(p, pl.remap, pl.mid_rows, pl.mid_cols, pl.out_rows, pl.out_cols);
  const int geom[11] = {pl.win_x, pl.win_y, pl.win_w, pl.win_h, pl.pic_x, pl.pic_y, pl.pic_w, pl.pic_h, pl.dl_rows, pl.dl_cols, pl.rsz_active ? 1 + pl.rsz_kind : 0};
  const size_t pitch = pitch16((size_t)pl.dl_cols);
  if (!(mh.valid && mh.base == key && mh.mode == mode && std::equal(geom, geom + 11, mh.geom))) {
    mh.valid = false;
    const ConstFrameView base = ensure_mask_base(p, pl.remap, pl.mid_rows, pl.mid_cols, pl.out_rows, pl.out_cols, binary && identity);
    mh.img.reserve(pitch * (size_t)pl.dl_rows);
    const FrameView dst = {mh.img.as<uint8_t>(), pitch, pitch * (size_t)pl.dl_rows, pl.dl_rows, pl.dl_cols};
    p->work_enqueued = true;
    if (identity) {
      HIP_CHECK(hipMemcpy2DAsync(dst.ptr, dst.step, base.ptr, base.step, (size_t)base.cols, (size_t)base.rows, hipMemcpyDeviceToDevice, p->stream));
    } else {
      const FrameView staged = {const_cast<uint8_t*>(base.ptr), base.step, base.frame_stride, base.rows, base.cols};  // read only
      const HeadPrep hp = prepare_head(p, pl, staged, 1);
      enqueue_head(p, pl, hp, staged, dst, 1, 0);
      if (binary) {
        LaunchLogScope log_scope(p);
        rip::MaskThresholdParams t = {dst.ptr, dst.step, dst.rows, dst.cols};
        rip::LaunchInfo info = {};
        launched(rip::launch_mask_threshold(t, p->stream, &info), info, "the mask threshold", 0);
      }
    }
    mh.base = key;
    mh.mode = mode;
    std::copy(geom, geom + 11, mh.geom);
    mh.valid = true;
    mh.builds++;
  }
  return {mh.img.as<uint8_t>(), pitch, pitch * (size_t)pl.dl_rows, pl.dl_rows, pl.dl_cols};
}

}  // namespace rip::api
