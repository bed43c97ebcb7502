// rip_api.cpp -- the C-ABI declared in include/rip.h, minus the host-frame calls (rip_ring.cpp) and the loaders, setters and
// getters (rip_settings.cpp): one handle owns the module parameters (rip_params.hpp), the device-resident constants and scratch;
// rip_apply_device enqueues the kernels of a batch on the caller's HIP stream (rip_batch.cpp).  There is no CPU execution path.
#include <algorithm>
#include <cstdarg>
#include <cstring>

#include "rip_handle.hpp"
#include "rip_unpack.hpp"

namespace rip {
// the launch record's sink (rip_kernels.hpp)
__thread LaunchLog* t_launch_log = nullptr;
void launch_log_add(LaunchLog* log, int fc, unsigned grid_x, unsigned grid_y, unsigned block, int frames, const char* fmt, ...) {
  char name[160], line[256];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(name, sizeof(name), fmt, ap);
  va_end(ap);
  std::snprintf(line, sizeof(line), "%s fc=%d grid=%u,%u block=%u frames=%d\n", name, fc, grid_x, grid_y, block, frames);
  log->text += line;
}

Tunables tunables_from_env() {
  Tunables t;
  auto positive = [](const char* name, int dflt) {
    const char* e = std::getenv(name);
    if (!e || !*e) return dflt;
    const int v = std::atoi(e);
    return v > 0 ? v : dflt;
  };
  t.chain_blocks = positive("RIP_CHAIN_BLOCKS", t.chain_blocks);
  t.chain_frames = positive("RIP_CHAIN_FRAMES", t.chain_frames);
  t.stats_blocks = positive("RIP_STATS_BLOCKS", t.stats_blocks);
  if (const char* e = std::getenv("RIP_REMAP_RING")) t.remap_ring = std::atoi(e) != 0;
  t.remap_stages = positive("RIP_REMAP_STAGES", t.remap_stages);
  t.remap_per_cu = positive("RIP_REMAP_PER_CU", t.remap_per_cu);
  t.remap_frames = positive("RIP_REMAP_FRAMES", t.remap_frames);
  t.remap_exp = positive("RIP_REMAP_EXP", t.remap_exp);
  if (const char* e = std::getenv("RIP_REMAP_DEAL")) t.remap_deal = std::max(0, std::atoi(e));
  if (const char* e = std::getenv("RIP_REMAP_ORDER")) t.remap_order = std::max(0, std::min(2, std::atoi(e)));
  if (const char* e = std::getenv("RIP_CHAIN_DEAL")) t.chain_deal = std::max(0, std::atoi(e));
  if (const char* e = std::getenv("RIP_REMAP_FUSED")) t.remap_fused = std::atoi(e) != 0;
  if (const char* e = std::getenv("RIP_CHAIN_FOOTPRINT")) t.chain_footprint = std::atoi(e) != 0;
  if (const char* e = std::getenv("RIP_CHAIN_NT")) t.chain_nt = std::atoi(e);
  t.ccc_lds_hist_min = positive("RIP_CCC_LDS_HIST_MIN", t.ccc_lds_hist_min);
  t.overlap_groups = positive("RIP_OVERLAP_GROUPS", t.overlap_groups);
  t.overlap_mode = positive("RIP_OVERLAP_MODE", t.overlap_mode);
  t.debug_occupancy = std::getenv("RIP_DEBUG_OCC") != nullptr;
  return t;
}
}  // namespace rip

// The body selects the handle's device and does not put the caller's back: the members' destructors run right behind it, so
// every DevBuf of the handle frees its memory under that device without being named here.
rip_pipeline::~rip_pipeline() {
  if (device < 0) return;
  (void)hipSetDevice(device);
  for (hipEvent_t e : prof_events) (void)hipEventDestroy(e);
  for (hipEvent_t e : ovl_events) (void)hipEventDestroy(e);
  if (switch_event) (void)hipEventDestroy(switch_event);
  if (aux_stream) (void)hipStreamDestroy(aux_stream);
  if (ul_stream) (void)hipStreamSynchronize(ul_stream);
  if (dl_stream) (void)hipStreamSynchronize(dl_stream);
  for (auto& sl : ring) sl->release();
  if (ul_stream) (void)hipStreamDestroy(ul_stream);
  if (dl_stream) (void)hipStreamDestroy(dl_stream);
}

namespace rip::api {

rip_status status_of(const std::exception& e) {
  if (dynamic_cast<const std::invalid_argument*>(&e)) return RIP_ERR_INVALID_ARGUMENT;  // InvalidArgument among them
  if (dynamic_cast<const AssertError*>(&e)) return RIP_ERR_ASSERT;
  if (dynamic_cast<const rip::YamlError*>(&e)) return RIP_ERR_IO;
  if (dynamic_cast<const CapacityError*>(&e)) return RIP_ERR_CAPACITY;
  return RIP_ERR_DEVICE;  // DeviceError and everything else
}

void need(const rip_pipeline* p) {
  if (!p) throw InvalidArgument("null pipeline handle");
}

void need_device(const rip_pipeline* p) {
  need(p);
  if (p->device == RIP_DEVICE_NONE)
    throw DeviceError("this handle was created with RIP_DEVICE_NONE (parameter handling only): frames can only be "
                      "processed on a HIP device; there is no CPU execution path");
}

void need_head(const rip_pipeline* p, int head) {
  if (head < 0 || head >= p->m.n_heads)
    throw InvalidArgument("output head " + std::to_string(head) + " does not exist: the handle has heads 0.." + std::to_string(p->m.n_heads - 1));
}

void copy_string(const std::string& s, char* out, size_t cap) {
  if (!out || cap == 0) throw InvalidArgument("null output buffer");
  if (s.size() + 1 > cap) throw CapacityError("string buffer too small");
  std::memcpy(out, s.c_str(), s.size() + 1);
}

Plan delivered_plan(const rip_pipeline* p, int rows, int cols, int channels, const char* encoding) {
  if (!encoding) throw InvalidArgument("encoding is null");
  Plan pl = make_plan(p->m, rows, cols, channels, encoding);
  apply_output_format(p->m, p->m.selected, pl);
  return pl;
}

}  // namespace rip::api

using namespace rip::api;

namespace {
// the white-balance records of the first n_frames of the last batch (rip_get_white_balance_info, rip_get_ccc_track)
std::vector<rip::FrameWb> download_wb(rip_pipeline* p, const void* out, int n_frames) {
  need(p);
  if (!out || n_frames <= 0) throw InvalidArgument("bad arguments");
  if (n_frames > p->last_batch_frames || !p->d_wb.ptr) throw InvalidArgument("no white-balance results for that many frames");
  need_device(p);
  DeviceGuard device_guard(p->device);
  std::vector<rip::FrameWb> h(n_frames);
  HIP_CHECK(hipMemcpyAsync(h.data(), p->d_wb.ptr, sizeof(rip::FrameWb) * n_frames, hipMemcpyDeviceToHost, p->stream));
  HIP_CHECK(hipStreamSynchronize(p->stream));
  return h;
}
thread_local std::string g_create_error;
}  // namespace

#pragma GCC visibility push(default)
extern "C" {

const char* rip_version(void) { return "raw_image_pipeline_amd 0.1 (gfx950)"; }

rip_status rip_create(int device, int use_gpu, const char* params_path, const char* calibration_path,
                      const char* color_calibration_path, rip_pipeline** out) {
  if (!out) {
    g_create_error = "rip_create: out is null";
    return RIP_ERR_INVALID_ARGUMENT;
  }
  *out = nullptr;
  rip_pipeline* p = nullptr;
  try {
    if (device != RIP_DEVICE_NONE) {
      int count = 0;
      hipError_t e = hipGetDeviceCount(&count);
      if (e != hipSuccess || count <= 0)
        throw DeviceError("no HIP device available: this library has no CPU execution path (hipGetDeviceCount: " +
                          std::string(hipGetErrorString(e)) + ")");
      if (device < 0 || device >= count) throw InvalidArgument("device ordinal out of range");
      HIP_CHECK(hipSetDevice(device));
    }
    p = new rip_pipeline();
    p->device = device;
    p->m.use_gpu = use_gpu != 0;
    // RawImagePipeline(use_gpu, params, calib, color_calib), raw_image_pipeline.cpp:23-40
    if (!params_path || !*params_path) {
      rip::apply_example_params(p->m);  // DEFAULT_PARAMS_PATH = config/pipeline_params_example.yaml
    } else if (!rip::load_params_file(p->m, params_path)) {
      std::fprintf(stderr, "Warning: parameters file doesn't exist\n");
    }
    if (calibration_path && *calibration_path) {
      if (!rip::load_camera_calibration_file(p->m, calibration_path)) std::fprintf(stderr, "Warning: Calibration file doesn't exist\n");
    }
    if (!color_calibration_path || !*color_calibration_path) {
      rip::apply_example_color_calibration(p->m);  // DEFAULT_COLOR_CALIBRATION_PATH
    } else if (!rip::load_color_calibration_file(p->m, color_calibration_path)) {
      std::fprintf(stderr, "Warning: Color calibration file doesn't exist\n");
    }
    und_init(p);
    // every environment override is read here, once per handle
    p->tn = rip::tunables_from_env();
    if (const char* t = std::getenv("RIP_REMAP_TILED")) p->use_tiled_remap = std::atoi(t) != 0;
    if (const char* e = std::getenv("RIP_MAPS_ON_HOST")) p->maps_on_host = *e && *e != '0';
    if (const char* e = std::getenv("RIP_PLAN_ON_HOST")) p->plan_on_host = *e && *e != '0';
    if (const char* e = std::getenv("RIP_DEBUG_DIR")) if (*e) p->debug_dir = e;
    if (const char* e = std::getenv("RIP_CCC_MODEL")) if (*e) p->ccc_model_env = e;
    if (const char* e = std::getenv("RIP_FP_CONTRACT")) {
      // the same values rip_set_fp_contraction accepts; anything else ("2", "true", a typo) fails the create instead of silently
      // selecting the x86 model
      if ((e[0] != '0' && e[0] != '1') || e[1] != 0) throw rip::YamlError(std::string("RIP_FP_CONTRACT=[") + e + "]: 0 (uncontracted) or 1 (contracted) expected");
      p->fp_contract = e[0] == '1' ? 1 : 0;
    }
    if (!p->ccc_model_env.empty()) rip::ccc_load_model_file(p->ccc.model, p->ccc_model_env);
    *out = p;
    return RIP_OK;
  } catch (const std::exception& e) {
    g_create_error = e.what();
    delete p;
    const rip_status st = status_of(e);  // a create fails for its files, its arguments or the device
    return st == RIP_ERR_IO || st == RIP_ERR_INVALID_ARGUMENT ? st : RIP_ERR_DEVICE;
  }
}

rip_status rip_create_default(int device, int use_gpu, rip_pipeline** out) {
  // RawImagePipeline(bool use_gpu), raw_image_pipeline.cpp:16-21: example params, example camera
  // calibration and example colour calibration
  rip_status st = rip_create(device, use_gpu, nullptr, nullptr, nullptr, out);
  if (st != RIP_OK) return st;
  rip::apply_example_camera_calibration((*out)->m);
  und_init(*out);
  return RIP_OK;
}

void rip_destroy(rip_pipeline* p) { delete p; }

const char* rip_last_error(const rip_pipeline* p) { return p ? p->last_error.c_str() : g_create_error.c_str(); }

rip_status rip_set_stream(rip_pipeline* p, void* s) {
  return guarded(p, [&] {
    need_device(p);
    hipStream_t next = static_cast<hipStream_t>(s);
    if (next != p->stream && p->work_enqueued) {
      // The handle's scratch state crosses frame calls in stream order (statistics records and ccc histogram counters handed
      // back zeroed by the kernels of the call before, the ccc Kalman state, the gains the debug dumps reuse): work left on
      // the old stream must come first on the new one too.  Best effort -- a stream the caller has destroyed already has
      // nothing pending and the runtime refuses the record, which is ignored.
      DeviceGuard device_guard(p->device);
      if (!p->switch_event && hipEventCreateWithFlags(&p->switch_event, hipEventDisableTiming) != hipSuccess) p->switch_event = nullptr;
      if (p->switch_event && hipEventRecord(p->switch_event, p->stream) == hipSuccess) (void)hipStreamWaitEvent(next, p->switch_event, 0);
      (void)hipGetLastError();
    }
    p->stream = next;
  });
}

rip_status rip_query_output(rip_pipeline* p, int rows, int cols, int channels, const char* encoding, int* out_rows,
                            int* out_cols, int* out_channels, char encoding_out[32]) {
  return guarded(p, [&] {
    need(p);
    const Plan pl = delivered_plan(p, rows, cols, channels, encoding);
    if (out_rows) *out_rows = pl.dl_rows;
    if (out_cols) *out_cols = pl.dl_cols;
    if (out_channels) *out_channels = pl.dl_channels;
    if (encoding_out) copy_string(pl.encoding_out, encoding_out, 32);
  });
}

rip_status rip_query_output_bytes(rip_pipeline* p, int rows, int cols, int channels, const char* encoding, size_t* bytes, int* elem_bytes,
                                  int* planar) {
  return guarded(p, [&] {
    need(p);
    const Plan pl = delivered_plan(p, rows, cols, channels, encoding);
    if (bytes) *bytes = delivered_bytes(pl);
    if (elem_bytes) *elem_bytes = pl.dl_elem_bytes;
    if (planar) *planar = pl.dl_planar ? 1 : 0;
  });
}

rip_status rip_query_taps(rip_pipeline* p, int rows, int cols, int channels, const char* encoding, int* tap_rows, int* tap_cols,
                          int* tap_channels) {
  return guarded(p, [&] {
    need(p);
    if (!encoding) throw InvalidArgument("encoding is null");
    Plan pl = make_plan(p->m, rows, cols, channels, encoding);
    if (tap_rows) *tap_rows = pl.mid_rows;
    if (tap_cols) *tap_cols = pl.mid_cols;
    if (tap_channels) *tap_channels = pl.channels;
  });
}

rip_status rip_apply_device(rip_pipeline* p, const void* d_in, size_t in_step, size_t in_frame_stride, int n_frames, int rows,
                            int cols, int channels, const char* encoding, void* d_out, size_t out_step,
                            size_t out_frame_stride, void* d_tap_debayered, void* d_tap_color) {
  return guarded(p, [&] {
    need_device(p);
    if (!d_in || !d_out || !encoding) throw InvalidArgument("null buffer or encoding");
    if (n_frames < 0) throw InvalidArgument("negative frame count");
    if (n_frames == 0) return;
    const Plan pl = delivered_plan(p, rows, cols, channels, encoding);  // a null encoding was refused above, in this call's words
    resolve_input_pitches(pl, rows, cols, channels, in_step, in_frame_stride);
    // bgr16 results (the 16-bit range is off); with a range the frame is an 8-bit one after the demosaic and keeps its taps
    if (pl.out_elem_bytes == 2 && (d_tap_debayered || d_tap_color)) throw InvalidArgument("16-bit Bayer frames have no taps");
    const FrameView dst = resolve_output_layout(pl, d_out, out_step, out_frame_stride);
    const ConstFrameView src = resolve_input_layout(pl, d_in, in_step, in_frame_stride, rows, cols, channels);
    const size_t tap_frame = (size_t)pl.mid_rows * pl.mid_cols * pl.channels;
    // several kernels put the frame index on gridDim.y (<= 65535): longer batches go through in slices.  The
    // frames of a stream are processed in order either way (the ccc Kalman state lives on the device).
    constexpr int kMaxFramesPerLaunch = 16384;
    begin_jpeg_call(p, pl, n_frames);
    for (int f0 = 0; f0 < n_frames; f0 += kMaxFramesPerLaunch) {
      const Taps taps = {d_tap_debayered ? static_cast<uint8_t*>(d_tap_debayered) + (size_t)f0 * tap_frame : nullptr,
                         d_tap_color ? static_cast<uint8_t*>(d_tap_color) + (size_t)f0 * tap_frame : nullptr};
      run_batch_formatted(p, pl, frames_from(src, f0), frames_from(dst, f0), taps, std::min(kMaxFramesPerLaunch, n_frames - f0), f0);
    }
    remember_mask_frame(p, pl);
  });
}

// ---- output heads --------------------------------------------------------------------------------
rip_status rip_debug_output_head_info(rip_pipeline* p, int head, int* table_builds, int* direct_write, int* copied) {
  return guarded(p, [&] {
    need(p);
    need_head(p, head);
    if (table_builds) *table_builds = p->out_table[head].builds + p->rsz_tables[head].builds;
    if (direct_write) *direct_write = p->head_record[head].direct_write;
    if (copied) *copied = p->head_record[head].copied;
  });
}

rip_status rip_apply_device_heads(rip_pipeline* p, const void* d_in, size_t in_step, size_t in_frame_stride, int n_frames, int rows, int cols,
                                  int channels, const char* encoding, const rip_head_buffer* heads, int n_heads, void* d_tap_debayered,
                                  void* d_tap_color) {
  return guarded(p, [&] {
    need_device(p);
    if (!d_in || !heads || !encoding) throw InvalidArgument("null buffer, heads or encoding");
    if (n_heads != p->m.n_heads)
      throw InvalidArgument("rip_apply_device_heads: " + std::to_string(n_heads) + " head buffers for a handle with " + std::to_string(p->m.n_heads) + " output heads");
    bool requested[RIP_MAX_OUTPUT_HEADS] = {};
    bool any = false;
    for (int k = 0; k < n_heads; k++) any |= requested[k] = heads[k].d_out != nullptr;
    if (!any) throw InvalidArgument("rip_apply_device_heads: no head is requested (every d_out is null)");
    if (n_frames < 0) throw InvalidArgument("negative frame count");
    if (n_frames == 0) return;
    const Plan pl = make_plan(p->m, rows, cols, channels, encoding);
    Plan plans[RIP_MAX_OUTPUT_HEADS];
    FrameView dsts[RIP_MAX_OUTPUT_HEADS];
    plan_heads(p->m, pl, n_heads, requested, d_tap_debayered || d_tap_color, plans, dsts,
               [&](int k, const Plan& hp) { return resolve_output_layout(hp, heads[k].d_out, heads[k].out_step, heads[k].out_frame_stride); });
    const ConstFrameView src = resolve_input_layout(pl, d_in, in_step, in_frame_stride, rows, cols, channels);  // rip_apply_device's rules
    const size_t tap_frame = (size_t)pl.mid_rows * pl.mid_cols * pl.channels;
    constexpr int kMaxFramesPerLaunch = 16384;  // rip_apply_device's slices: per slice the chain runs once, then the heads
    for (int k = 0; k < n_heads; k++)
      if (requested[k]) begin_jpeg_call(p, plans[k], n_frames);
    for (int f0 = 0; f0 < n_frames; f0 += kMaxFramesPerLaunch) {
      const Taps taps = {d_tap_debayered ? static_cast<uint8_t*>(d_tap_debayered) + (size_t)f0 * tap_frame : nullptr,
                         d_tap_color ? static_cast<uint8_t*>(d_tap_color) + (size_t)f0 * tap_frame : nullptr};
      FrameView slice[RIP_MAX_OUTPUT_HEADS];
      for (int k = 0; k < n_heads; k++) slice[k] = requested[k] ? frames_from(dsts[k], f0) : dsts[k];
      run_batch_heads(p, pl, plans, slice, n_heads, frames_from(src, f0), taps, std::min(kMaxFramesPerLaunch, n_frames - f0), f0);
    }
    remember_mask_frame(p, pl);
  });
}

// ---- the stream lengths of a "jpeg" head -----------------------------------------------------------
rip_status rip_get_output_jpeg_sizes(rip_pipeline* p, uint32_t* sizes, int capacity, int* n) {
  return guarded(p, [&] {
    need_device(p);
    const int head = p->m.selected, frames = p->jpeg_frames[head];
    if (n) *n = frames;
    if (!sizes) return;  // the count only
    if (capacity < frames) throw CapacityError("jpeg sizes: room for " + std::to_string(frames) + " frames is needed");
    DeviceGuard device_guard(p->device);
    if (frames) HIP_CHECK(hipMemcpyAsync(sizes, p->d_jpeg_sizes[head].ptr, (size_t)frames * 4, hipMemcpyDeviceToHost, p->stream));
    HIP_CHECK(hipStreamSynchronize(p->stream));
  });
}

rip_status rip_get_output_jpeg_sizes_device(rip_pipeline* p, const uint32_t** d_sizes, int* n) {
  return guarded(p, [&] {
    need_device(p);
    if (!d_sizes) throw InvalidArgument("null sizes pointer");
    const int head = p->m.selected;
    *d_sizes = p->jpeg_frames[head] ? p->d_jpeg_sizes[head].as<uint32_t>() : nullptr;
    if (n) *n = p->jpeg_frames[head];
  });
}

rip_status rip_debug_jpeg_tables(int quality, uint8_t* q, uint32_t* recip, uint32_t* half) {
  return guarded(static_cast<const rip_pipeline*>(nullptr), [&] {
    rip::check_output_jpeg(quality, 1);
    if (!q || !recip || !half) throw InvalidArgument("rip_debug_jpeg_tables: null argument");
    rip::JpegTables t;
    rip::jpeg_build_tables(quality, t, q);
    std::memcpy(recip, t.recip, sizeof(t.recip));
    std::memcpy(half, t.half, sizeof(t.half));
  });
}

// ---- valid-pixel masks ---------------------------------------------------------------------------
// rip_get_output_mask / rip_get_output_mask_device up to the geometry: the refusals in their order (the mode, then exactly those of
// rip_query_output), nothing enqueued
static Plan output_mask_plan(rip_pipeline* p, int rows, int cols, int channels, const char* encoding, int* mode) {
  need(p);
  *mode = rip::rect_mask_mode_id(p->m.rect_mask);
  if (*mode == 0) throw InvalidArgument("the rect mask mode is 'off': no masks are built (rip_set_rect_mask 'coverage' or 'valid')");
  return delivered_plan(p, rows, cols, channels, encoding);
}

rip_status rip_get_output_mask(rip_pipeline* p, int rows, int cols, int channels, const char* encoding, uint8_t* out, size_t capacity,
                               int* height, int* width) {
  return guarded(p, [&] {
    int mode = 0;
    const Plan pl = output_mask_plan(p, rows, cols, channels, encoding, &mode);
    const size_t bytes = (size_t)pl.img_rows * (size_t)pl.dl_pic_cols;  // a mask is the picture's, whatever the format
    if (out && capacity < bytes) throw CapacityError("mask buffer too small: need " + std::to_string(bytes) + " bytes");
    if (height) *height = pl.img_rows;
    if (width) *width = pl.dl_pic_cols;
    if (!out) return;  // the geometry only
    need_device(p);
    DeviceGuard device_guard(p->device);
    const ConstFrameView m = ensure_mask_head(p, pl, mode);
    HIP_CHECK(hipMemcpy2DAsync(out, (size_t)m.cols, m.ptr, m.step, (size_t)m.cols, (size_t)m.rows, hipMemcpyDeviceToHost, p->stream));
    HIP_CHECK(hipStreamSynchronize(p->stream));
  });
}

rip_status rip_get_output_mask_device(rip_pipeline* p, int rows, int cols, int channels, const char* encoding, const uint8_t** d_mask,
                                      size_t* pitch, int* height, int* width) {
  return guarded(p, [&] {
    int mode = 0;
    const Plan pl = output_mask_plan(p, rows, cols, channels, encoding, &mode);
    if (!d_mask) throw InvalidArgument("null mask pointer");
    need_device(p);
    const ConstFrameView m = ensure_mask_head(p, pl, mode);
    *d_mask = m.ptr;
    if (pitch) *pitch = m.step;
    if (height) *height = m.rows;
    if (width) *width = m.cols;
  });
}

rip_status rip_debug_rect_mask_info(rip_pipeline* p, int head, int* mask_builds, int* head_builds) {
  return guarded(p, [&] {
    need(p);
    need_head(p, head);
    if (mask_builds) *mask_builds = p->mask_base.builds;
    if (head_builds) *head_builds = p->mask_head[head].builds;
  });
}

rip_status rip_init_undistortion(rip_pipeline* p) {
  return guarded(p, [&] {
    need(p);
    und_init(p);
    ensure_host_maps(p);
    if (p->device != RIP_DEVICE_NONE) {
      DeviceGuard device_guard(p->device);
      ensure_maps(p);
    }
  });
}
rip_status rip_debug_output_window(int cols, int rows, const int roi_xywh[4], int width, int height, const char* fit, int src_xywh[4], int dst_xywh[4]) {
  return guarded(static_cast<const rip_pipeline*>(nullptr), [&] {
    if (!roi_xywh || !fit || !src_xywh || !dst_xywh) throw InvalidArgument("rip_debug_output_window: null argument");
    if (cols < 1 || rows < 1) throw InvalidArgument("rip_debug_output_window: empty image");
    rip::check_output_roi(roi_xywh[0], roi_xywh[1], roi_xywh[2], roi_xywh[3]);
    rip::check_output_size(width, height);
    rip::output_window_geometry(cols, rows, roi_xywh, width, height, rip::output_fit_id(fit), src_xywh, dst_xywh);
  });
}

rip_status rip_debug_resize_tables(int src_rows, int src_cols, int dst_rows, int dst_cols, int32_t* xofs, int16_t* alpha, int32_t* yofs, int16_t* beta,
                                   int* area2) {
  return guarded(static_cast<const rip_pipeline*>(nullptr), [&] {
    rip::build_resize_tables(src_rows, src_cols, dst_rows, dst_cols, xofs, alpha, yofs, beta, area2);
  });
}

rip_status rip_debug_resize_area_tables(int src_rows, int src_cols, int dst_rows, int dst_cols, int32_t* xfirst, int32_t* xcount, float* xweight,
                                        int32_t* yfirst, int32_t* ycount, float* yweight, int* whole, float* scale) {
  return guarded(static_cast<const rip_pipeline*>(nullptr), [&] {
    rip::build_resize_area_tables(src_rows, src_cols, dst_rows, dst_cols, xfirst, xcount, xweight, yfirst, ycount, yweight, whole, scale);
  });
}

rip_status rip_debug_resize_aa_tables(const char* name, int src_rows, int src_cols, int dst_rows, int dst_cols, int channels, int32_t* xfirst,
                                      int32_t* xcount, int32_t* xwofs, int16_t* xweight, int32_t* yfirst, int32_t* ycount, int32_t* ywofs, int16_t* yweight,
                                      int* xprec, int* yprec, int* tile_rows, int* lds_rows) {
  return guarded(static_cast<const rip_pipeline*>(nullptr), [&] {
    if (!name) throw InvalidArgument("rip_debug_resize_aa_tables: null name");
    const int filter = rip::output_interpolation_id(name);
    if (filter < 2) throw InvalidArgument("rip_debug_resize_aa_tables: \"linear_aa\" or \"cubic_aa\"");
    if (channels != 1 && channels != 3) throw InvalidArgument("rip_debug_resize_aa_tables: 1 or 3 channels");
    int th[2] = {0, 0}, lr[2] = {0, 0};
    rip::build_resize_aa_tables(filter, src_rows, src_cols, dst_rows, dst_cols, xfirst, xcount, xwofs, xweight, xprec, yfirst, ycount, ywofs, yweight, yprec,
                                th, lr);
    if (tile_rows) *tile_rows = th[channels == 3];
    if (lds_rows) *lds_rows = lr[channels == 3];
  });
}

rip_status rip_debug_output_table(const char* name, double divisor, const double* mean, const double* sd, void* out) {
  return guarded(static_cast<const rip_pipeline*>(nullptr), [&] {
    if (!name || !mean || !sd || !out) throw InvalidArgument("rip_debug_output_table: null argument");
    const int fmt = rip::output_format_id(name);
    rip::build_output_table(fmt, divisor, mean, sd, out);
  });
}

rip_status rip_debug_raw16_narrow(int black, int white, const uint16_t* in, uint8_t* out, size_t n) {
  return guarded(static_cast<const rip_pipeline*>(nullptr), [&] {
    rip::check_debayer_16bit_range(black, white);
    if ((black == 0 && white == 0) || (n && (!in || !out))) throw InvalidArgument("rip_debug_raw16_narrow: a range and buffers are needed");
    uint32_t mul;
    int shift;
    rip::raw16_narrow_constants(black, white, &mul, &shift);
    const int range = white - black;
    for (size_t i = 0; i < n; i++) {  // Narrow::operator() of rip_raw16.hip, statement for statement
      const int t = std::min(std::max((int)in[i] - black, 0), range);
      const uint32_t num = (uint32_t)t * 510u + (uint32_t)range;
      out[i] = (uint8_t)((uint32_t)(((uint64_t)(num << 6) * mul) >> 32) >> shift);
    }
  });
}

rip_status rip_debug_unpack(const char* encoding, const uint8_t* in, size_t step, int rows, int cols, uint16_t* out) {
  return guarded(static_cast<const rip_pipeline*>(nullptr), [&] {
    int ry, rx;
    const int layout = encoding ? parse_packed(encoding, ry, rx) : 0;
    if (!layout) throw InvalidArgument("rip_debug_unpack: not a packed Bayer encoding");
    if (rows < 0 || cols < 0 || (rows && cols && (!in || !out))) throw InvalidArgument("rip_debug_unpack: buffers are needed");
    const int mult = rip::packed_cols_multiple(layout);
    if (cols % mult != 0) throw InvalidArgument("rip_debug_unpack: the width must be a multiple of " + std::to_string(mult));
    const size_t in_row = rip::packed_row_bytes(layout, cols);
    if (step == 0) step = in_row;
    if (step < in_row) throw InvalidArgument("input row pitch smaller than a row");
    for (int y = 0; y < rows; y++) {
      const uint8_t* row = in + (size_t)y * step;
      uint16_t* o = out + (size_t)y * cols;
      for (int x = 0; x < cols; x++) {  // StagePacked::sample of rip_raw16_dev.hpp: the same functions of rip_unpack.hpp
        switch (layout) {
          case rip::PACKED_10P: o[x] = (uint16_t)rip::unpack_sample<rip::PACKED_10P>(row, x); break;
          case rip::PACKED_12P: o[x] = (uint16_t)rip::unpack_sample<rip::PACKED_12P>(row, x); break;
          case rip::PACKED_10_CSI2: o[x] = (uint16_t)rip::unpack_sample<rip::PACKED_10_CSI2>(row, x); break;
          default: o[x] = (uint16_t)rip::unpack_sample<rip::PACKED_12_CSI2>(row, x); break;
        }
      }
    }
  });
}

// ---- introspection -------------------------------------------------------------------------------
rip_status rip_get_undistortion_maps(rip_pipeline* p, float* map_x, float* map_y, size_t cap, int* rows, int* cols) {
  return guarded(p, [&] {
    need(p);
    if (rows) *rows = p->m.dist_h;
    if (cols) *cols = p->m.dist_w;
    if (!map_x || !map_y) return;
    need_host_map(p);
    size_t n = (size_t)p->m.dist_w * p->m.dist_h;
    if (cap < n) throw CapacityError("map buffers too small");
    for (size_t i = 0; i < n; i++) {
      map_x[i] = p->maps.host[2 * i];
      map_y[i] = p->maps.host[2 * i + 1];
    }
  });
}

rip_status rip_get_white_balance_info(rip_pipeline* p, float* out, int n_frames) {
  return guarded(p, [&] {
    const std::vector<rip::FrameWb> h = download_wb(p, out, n_frames);
    for (int f = 0; f < n_frames; f++) {
      float* o = out + 8 * f;
      o[0] = h[f].fg[0]; o[1] = h[f].fg[1]; o[2] = h[f].fg[2];
      o[3] = (float)h[f].q8[0]; o[4] = (float)h[f].q8[1]; o[5] = (float)h[f].q8[2];
      o[6] = (float)h[f].uv[0]; o[7] = (float)h[f].uv[1];
    }
  });
}

rip_status rip_get_ccc_track(rip_pipeline* p, int* out, int n_frames) {
  return guarded(p, [&] {
    const std::vector<rip::FrameWb> h = download_wb(p, out, n_frames);
    for (int f = 0; f < n_frames; f++) {
      out[4 * f + 0] = h[f].uv_raw[0];
      out[4 * f + 1] = h[f].uv_raw[1];
      out[4 * f + 2] = h[f].uv[0];
      out[4 * f + 3] = h[f].uv[1];
    }
  });
}

rip_status rip_profile_begin(rip_pipeline* p, int max_records) {
  return guarded(p, [&] {
    need_device(p);
    DeviceGuard device_guard(p->device);
    if (max_records < 0) throw InvalidArgument("negative record count");
    while (p->prof_events.size() < (size_t)max_records * 2) {
      hipEvent_t e;
      HIP_CHECK(hipEventCreate(&e));
      p->prof_events.push_back(e);
    }
    p->prof_used = 0;
    p->prof_ids.clear();
    p->prof_on = max_records > 0;
  });
}

rip_status rip_profile_end(rip_pipeline* p, double ms_sum[RIP_KERNEL_COUNT], int count[RIP_KERNEL_COUNT]) {
  return guarded(p, [&] {
    need_device(p);
    DeviceGuard device_guard(p->device);
    HIP_CHECK(hipStreamSynchronize(p->stream));
    for (int i = 0; i < RIP_KERNEL_COUNT; i++) {
      if (ms_sum) ms_sum[i] = 0;
      if (count) count[i] = 0;
    }
    for (size_t r = 0; r < p->prof_ids.size(); r++) {
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, p->prof_events[2 * r], p->prof_events[2 * r + 1]));
      if (ms_sum) ms_sum[p->prof_ids[r]] += ms;
      if (count) count[p->prof_ids[r]]++;
    }
    p->prof_on = false;
    p->prof_used = 0;
    p->prof_ids.clear();
  });
}

rip_status rip_debug_launch_log(rip_pipeline* p, int enable) {
  return guarded(p, [&] {
    need(p);
    if (enable) p->launch_log.text.clear();
    p->launch_log_on = enable != 0;
  });
}

rip_status rip_debug_get_launch_log(rip_pipeline* p, char* out, size_t capacity, size_t* needed) {
  return guarded(p, [&] {
    need(p);
    const std::string& t = p->launch_log.text;
    if (needed) *needed = t.size() + 1;
    if (capacity < t.size() + 1) throw CapacityError("launch log: " + std::to_string(t.size() + 1) + " bytes needed");
    if (!out) throw InvalidArgument("null buffer");
    std::memcpy(out, t.c_str(), t.size() + 1);
  });
}

rip_status rip_debug_write_png(rip_pipeline* p, const char* path, const uint8_t* image, int rows, int cols, int channels, int normalize) {
  return guarded(p, [&] {
    if (!path || !image) throw InvalidArgument("null path or image");
    if (rows < 1 || cols < 1 || (channels != 1 && channels != 3)) throw InvalidArgument("PNG dumps hold 1- or 3-channel 8-bit images");
    std::vector<uint8_t> tmp(image, image + (size_t)rows * cols * channels);
    if (normalize) rip::normalize_minmax_u8(tmp.data(), tmp.size());
    if (!rip::write_png(path, tmp.data(), rows, cols, channels)) throw rip::YamlError(std::string("cannot write ") + path);
  });
}

rip_status rip_debug_plan_info(rip_pipeline* p, int src_rows, int src_cols, int info[9]) {
  return guarded(p, [&] {
    need_device(p);
    if (!info) throw InvalidArgument("null info");
    DeviceGuard device_guard(p->device);
    ensure_plan(p, src_rows, src_cols);
    info[0] = p->plan.host.tiles_x;
    info[1] = p->plan.host.tiles_y;
    info[2] = p->plan.n_border;
    info[3] = (int)p->plan.host.max_lds_bytes;
    info[4] = p->plan.host.max_rect_w;
    info[5] = p->plan.host.max_rect_h;
    info[6] = p->plan.on_device ? 1 : 0;
    info[7] = rip::kRemapTileW;
    info[8] = rip::kRemapTileH;
  });
}

rip_status rip_debug_chain_footprint(rip_pipeline* p, int src_rows, int src_cols, int flip_angle, int info[4], int* intervals,
                                     int capacity_pairs) {
  return guarded(p, [&] {
    need(p);
    if (!info) throw InvalidArgument("null info");
    if (flip_angle != 0 && flip_angle != 180) throw InvalidArgument("the footprint walk serves flips of 0 and 180 degrees");
    if (src_rows < 2 || src_cols < 4 || src_rows % 2 || src_cols % 4 || src_rows / 2 > 65535 || src_cols / 4 > 65535)
      throw InvalidArgument("the footprint walk needs an even number of rows and a multiple of 4 columns");
    const int pairs = src_rows / 2, groups = src_cols / 4;
    if (intervals && capacity_pairs < pairs) throw InvalidArgument("intervals: one (lo, hi) per row pair");
    std::vector<int> lo, hi;
    if (p->device == RIP_DEVICE_NONE) {  // no plan on such a handle: the host compiler's footprint of the host-built maps
      ensure_host_maps(p);
      rip::compile_remap_footprint(p->maps.host.data(), p->m.dist_h, p->m.dist_w, src_rows, src_cols, lo, hi);
    } else {
      DeviceGuard device_guard(p->device);
      ensure_plan(p, src_rows, src_cols);
      lo = p->plan.host.fp_lo;
      hi = p->plan.host.fp_hi;
    }
    std::vector<uint32_t> items;
    rip::chain_footprint_items(lo, hi, src_rows, src_cols, flip_angle, items);
    int touched = 0;
    for (size_t i = 0; i < lo.size(); i++) touched += lo[i] < hi[i] ? 1 : 0;
    info[0] = pairs * groups;
    info[1] = (int)items.size();
    info[2] = touched;
    info[3] = p->last_chain_walked;
    if (intervals) {
      for (int i = 0; i < pairs; i++) intervals[2 * i] = intervals[2 * i + 1] = 0;
      for (size_t k = 0; k < items.size(); k++) {  // each pair's items are one run [lo, hi) in ascending order
        const int pr = (int)(items[k] >> 16), g = (int)(items[k] & 0xFFFFu);
        if (k == 0 || (int)(items[k - 1] >> 16) != pr) intervals[2 * pr] = g;
        intervals[2 * pr + 1] = g + 1;
      }
    }
  });
}

rip_status rip_debug_atan(rip_pipeline* p, const double* in, double* out, int n) {
  if (!p) return RIP_ERR_INVALID_ARGUMENT;
  return guarded(p, [&] {
    need_device(p);
    if (!in || !out || n < 0) throw InvalidArgument("bad arguments");
    DeviceGuard device_guard(p->device);
    DevBuf a, b;
    a.reserve((size_t)n * 8 + 8);
    b.reserve((size_t)n * 8 + 8);
    HIP_CHECK(hipMemcpyAsync(a.ptr, in, (size_t)n * 8, hipMemcpyHostToDevice, p->stream));
    rip::launch_atan_probe(a.as<double>(), b.as<double>(), n, p->stream);
    HIP_CHECK(hipMemcpyAsync(out, b.ptr, (size_t)n * 8, hipMemcpyDeviceToHost, p->stream));
    HIP_CHECK(hipStreamSynchronize(p->stream));
  });
}

rip_status rip_get_vignetting_mask(rip_pipeline* p, int rows, int cols, float* out, size_t capacity_floats) {
  if (!p) return RIP_ERR_INVALID_ARGUMENT;
  return guarded(p, [&] {
    if (rows < 1 || cols < 1 || !out || capacity_floats < (size_t)rows * cols) throw InvalidArgument("vignetting mask: bad size / buffer");
    std::vector<float> m;
    rip::build_vignette_mask(rows, cols, p->m.vig_scale, p->m.vig_a2, p->m.vig_a4, m, p->fp_contract);
    std::memcpy(out, m.data(), m.size() * sizeof(float));
  });
}

rip_status rip_debug_hbm_probe(rip_pipeline* p, int kind, size_t bytes, int reps, double* gbps) {
  return guarded(p, [&] {
    need_device(p);
    if (!gbps) throw InvalidArgument("null result pointer");
    if (kind < RIP_PROBE_COPY || kind > RIP_PROBE_EXPAND13_COALESCED_NT) throw InvalidArgument("unknown probe kind");
    bytes = bytes / 48 * 48;
    if (kind == RIP_PROBE_EXPAND13_COALESCED || kind == RIP_PROBE_EXPAND13_COALESCED_NT) bytes = bytes / 3072 * 3072;  // whole waves of 16-byte lanes
    if (bytes < 48 || reps < 1) throw InvalidArgument("rip_debug_hbm_probe: at least 48 bytes and one repetition");
    DeviceGuard device_guard(p->device);
    DevBuf src, dst;
    const bool expands = kind == RIP_PROBE_EXPAND13 || kind == RIP_PROBE_EXPAND13_NT || kind == RIP_PROBE_EXPAND13_WIDE || kind == RIP_PROBE_EXPAND13_WIDE_NT ||
                         kind == RIP_PROBE_EXPAND13_COALESCED || kind == RIP_PROBE_EXPAND13_COALESCED_NT;
    struct Events {
      hipEvent_t e0 = nullptr, e1 = nullptr;
      ~Events() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
      }
    } ev;
    if (kind != RIP_PROBE_FILL) {
      src.reserve(bytes);
      HIP_CHECK(hipMemsetAsync(src.ptr, 0x3c, bytes, p->stream));
    }
    dst.reserve(expands ? 3 * bytes : bytes);
    HIP_CHECK(hipEventCreate(&ev.e0));
    HIP_CHECK(hipEventCreate(&ev.e1));
    size_t moved = rip::launch_hbm_probe(kind, src.ptr, dst.ptr, bytes, p->stream);  // warm-up: page tables, caches, clocks
    HIP_CHECK(hipGetLastError());
    float best = 0.f;
    for (int r = 0; r < reps; r++) {
      HIP_CHECK(hipEventRecord(ev.e0, p->stream));
      moved = rip::launch_hbm_probe(kind, src.ptr, dst.ptr, bytes, p->stream);
      HIP_CHECK(hipEventRecord(ev.e1, p->stream));
      HIP_CHECK(hipEventSynchronize(ev.e1));
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
      if (ms > 0.f && (best == 0.f || ms < best)) best = ms;
    }
    *gbps = best > 0.f ? (double)moved / (best * 1e-3) / 1e9 : 0.0;
  });
}

int rip_get_table(rip_pipeline* p, int which, int32_t* out, int cap) {
  if (!p || !out) return -1;
  const rip::ColorTables& c = rip::color_tables();
  int n = 0;
  auto put = [&](auto* tab, int cnt) {
    n = cnt;
    for (int i = 0; i < cnt && i < cap; i++) out[i] = (int32_t)tab[i];
  };
  switch (which) {
    case 0: put(c.srgb_gamma, 256); break;
    case 1: put(c.cbrt, 3072); break;
    case 2: put(c.lab_to_yf, 512); break;
    case 3: put(c.inv_gamma, 4096); break;
    case 4: put(c.fwd, 9); break;
    case 5: put(c.inv, 9); break;
    case 6: put(c.sdiv, 256); break;
    case 7: put(c.hdiv180, 256); break;
    case 8: {
      uint8_t lut[256];
      rip::build_gamma_lut(p->m.gamma_k, lut);
      put(lut, 256);
      break;
    }
    default: return -1;
  }
  return n;
}

}  // extern "C"
#pragma GCC visibility pop

