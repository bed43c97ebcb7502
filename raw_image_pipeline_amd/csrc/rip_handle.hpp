// rip_handle.hpp -- internal to librip_hip.so (not installed): the handle behind include/rip.h and what the host units
// share.  rip_plan.cpp turns a frame's geometry and encoding into a Plan, rip_constants.cpp keeps the device-resident constants
// current and says what a setting invalidates, rip_batch.cpp enqueues the kernels of a batch, rip_output_stage.cpp those of the
// output stage behind it, rip_ring.cpp holds the host-frame calls and their ring, rip_settings.cpp the loaders, setters and
// getters, rip_api.cpp the rest of the C ABI.  Below the handle, without any HIP call and one header each behind rip_host.hpp:
// rip_yaml (the config files' reader), rip_params (module parameters, loaders, the checks of the settings), rip_output_tables
// (output table, window geometry, resize tables), rip_color_tables (gamma, Lab / HSV, vignetting), rip_undistort (maps, remap
// plan, footprint), rip_ccc_model (model spectra, host FFT) and rip_png (debug dumps).
#pragma once
#include "../../include/rip.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "rip_host.hpp"
#include "rip_kernels.hpp"
#include "rip_output.hpp"
#include "rip_aa.hpp"
#include "rip_clahe.hpp"
#include "rip_area.hpp"
#include "rip_fit.hpp"
#include "rip_heads.hpp"
#include "rip_jpeg.hpp"
#include "rip_mask.hpp"
#include "rip_resize.hpp"
#include "rip_yuv.hpp"

namespace rip {
// Launch record (rip_kernels.hpp): the text of a handle's log, one launch per line
struct LaunchLog {
  std::string text;
};
}  // namespace rip

namespace rip::api {

struct InvalidArgument : std::invalid_argument {
  using std::invalid_argument::invalid_argument;
};
struct AssertError : std::runtime_error {
  using std::runtime_error::runtime_error;
};
struct DeviceError : std::runtime_error {
  using std::runtime_error::runtime_error;
};
struct CapacityError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define HIP_CHECK(expr)                                                                                  \
  do {                                                                                                   \
    hipError_t err_ = (expr);                                                                            \
    if (err_ != hipSuccess)                                                                              \
      throw ::rip::api::DeviceError(std::string(#expr) + " failed: " + hipGetErrorString(err_) + " (" + __FILE__ + \
                        ":" + std::to_string(__LINE__) + ")");                                           \
  } while (0)

// Grow-only device buffer; frees its memory when it goes out of scope (on the device that is current then: ~rip_pipeline
// selects the handle's device before its members go)
struct DevBuf {
  void* ptr = nullptr;
  size_t cap = 0;
  // the leading bytes known to be zero, for the owners that track it (d_stats, d_hist); a new allocation knows nothing
  size_t clean_bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void reserve(size_t bytes) {
    if (bytes <= cap) return;
    if (ptr) HIP_CHECK(hipFree(ptr));
    ptr = nullptr;
    cap = 0;
    clean_bytes = 0;
    size_t want = bytes + bytes / 8;
    HIP_CHECK(hipMalloc(&ptr, want));
    cap = want;
    // RIP_TRACE_ALLOC=1: one line per device allocation on stderr (tools/probes/remap_modes_probe.py relates the per-process
    // modes of the remap's duration to where its buffers landed)
    static const bool trace = std::getenv("RIP_TRACE_ALLOC") != nullptr;
    if (trace) std::fprintf(stderr, "rip alloc %zu bytes at %p\n", want, ptr);
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
    clean_bytes = 0;
  }
  template <typename T>
  T* as() const {
    return static_cast<T*>(ptr);
  }
};

// Selects the handle's device for the duration of one C-ABI call and puts the caller's current device back afterwards
// (a CameraRig thread, or torch, keeps its own current device across calls into handles that live elsewhere).
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    HIP_CHECK(hipSetDevice(device));
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// What one frame geometry/encoding turns into
struct Plan {
  int src_kind = rip::SRC_BGR, ry = 0, rx = 0;
  int in_elem_bytes = 1;   // bytes per input sample: 2 for bayer_*16 frames (rip_set_debayer_16bit)
  int out_elem_bytes = 1;  // bytes per output sample: 2 = the 16-bit extension with the range off (debayer + flip only, bgr16 out)
  // bayer_*16 frames with a 16-bit range (rip_set_debayer_16bit_range): demosaiced at 16 bits, narrowed to 8 bits with
  // (black, white) and flipped by one pass of its own (rip_raw16.hip), then the whole chain as for a bgr8 frame
  bool raw16 = false;
  int black = 0, white = 0;
  // packed 10- / 12-bit frames (rip::PackedLayout; 0: none): a raw16 plan whose rows are unpacked by the kernel's tile staging
  // (rip_packed.hip), with the handle's range or the format's natural one
  int packed_layout = 0;
  bool mht = false;       // Bayer input demosaiced by Malvar-He-Cutler (rip_set_debayer_method "mht") instead of bilinear
  int channels = 3;       // channels after the debayer stage
  int flip_angle = 0;     // effective
  int mid_rows = 0, mid_cols = 0;  // post-flip geometry (pointwise chain output)
  int out_rows = 0, out_cols = 0;
  bool remap = false;
  int wb_mode = rip::WB_NONE;
  int stage_bits = 0;
  std::string encoding_out;
  // the output stage (rip_set_output_format; filled in by apply_output_format, everything above describes the pipeline's own image)
  int head = 0;                   // the output head whose settings these are (rip_select_output_head): its tables are the ones the launches read
  bool fmt_active = false;      // a format other than "native" is set
  int out_fmt = rip::OUT_NATIVE;  // the conversion that runs behind the last kernel; OUT_NATIVE: none (mono8 of a one-channel image included)
  int dl_channels = 3;            // what the frame calls deliver: channels (planes), bytes per element, planar or interleaved
  int dl_elem_bytes = 1;
  bool dl_planar = false;
  // the resize stage (rip_set_output_size; filled in by apply_output_format too): the delivered rows x cols -- out_rows / out_cols
  // stay the pipeline's own image F -- and whether a resize kernel runs between F and the converter (a target other than F's size)
  int dl_rows = 0, dl_cols = 0;
  // rows of the PICTURE F' that is delivered (what the resize writes and the converter reads; dl_cols is its width): dl_rows, except
  // under a YUV 4:2:0 format, whose delivered one-channel buffer has 3 * img_rows / 2 rows (rip_yuv.hpp)
  int img_rows = 0;
  int yuv_matrix = 0;  // rip::output_yuv_matrix_id of the head's matrix; read under OUT_NV12 / OUT_I420 only
  bool rsz_active = false;
  // which filter's kernel that is, as rip::output_interpolation_id numbers them: 0 the linear path's (also the exact 2 x 2 case under
  // "area", which is its mean kernel, and a copy under any name), 1 the area interpolation's (rip_area.hpp), 2 / 3 the antialiased
  // linear / cubic filter's (rip_aa.hpp)
  int rsz_kind = 0;
  // the window and the fit mode (rip_set_output_roi, rip_set_output_fit; rip::output_window_geometry): win_* is the rectangle of F
  // the resize reads, pic_* the rectangle of the delivered img_rows x dl_cols picture it writes; every other delivered pixel gets `pad`
  // (channels bytes).  fit_geometry: a window or a fit mode other than "stretch" is set, so these fields decide (without either
  // the window is F, the picture is the delivered image and the code paths are the ones from before there was a window).
  bool fit_geometry = false;
  int win_x = 0, win_y = 0, win_w = 0, win_h = 0;
  int pic_x = 0, pic_y = 0, pic_w = 0, pic_h = 0;
  uint8_t pad[4] = {0, 0, 0, 0};
  // CLAHE on the delivered one-channel picture (rip_set_output_clahe), the last launches of the head; such a head does not deliver F
  // as it is.  Off: the three other fields are not read.
  bool clahe = false;
  int clahe_tx = 0, clahe_ty = 0;
  double clahe_clip = 0.0;
  // the format "jpeg" (rip_set_output_jpeg; read under OUT_JPEG only): the delivered buffer is one row of dl_cols bytes, the default
  // slot; the picture that is coded is img_rows x dl_pic_cols of `channels` channels
  int jpeg_quality = 90, jpeg_restart_rows = 1;
  int dl_pic_cols = 0;  // the width of the delivered picture F': dl_cols, except under "jpeg", whose dl_cols is the slot
  bool win_is_frame() const { return win_x == 0 && win_y == 0 && win_w == out_cols && win_h == out_rows; }
  bool pic_is_delivered() const { return pic_w == dl_pic_cols && pic_h == img_rows; }
};

// n frames of rows x cols pixels in device memory: rows `step` bytes apart, frames `frame_stride` bytes apart (both resolved,
// never 0).  FrameView is written, ConstFrameView is read.
struct ConstFrameView {
  const uint8_t* ptr;
  size_t step, frame_stride;
  int rows, cols;
};
struct FrameView {
  uint8_t* ptr;
  size_t step, frame_stride;
  int rows, cols;
  operator ConstFrameView() const { return {ptr, step, frame_stride, rows, cols}; }
};
// bytes of a row rounded up to 16: the pitch of the staging images and of the masks
inline size_t pitch16(size_t row_bytes) { return (row_bytes + 15) & ~(size_t)15; }
// the view from frame f0 on
template <typename View>
View frames_from(View v, int f0) {
  v.ptr += (size_t)f0 * v.frame_stride;
  return v;
}
// the caller's tap buffers (null: not requested): tightly packed mid_rows x mid_cols x channels frames
struct Taps {
  uint8_t* debayered;
  uint8_t* color;
};

// One frame in flight on the asynchronous host path (rip_submit / rip_collect): its own device input / output / tap
// buffers, a pinned result buffer, and the three events that chain upload -> kernels -> download.
struct RingSlot {
  DevBuf d_in, d_out, d_tap_deb, d_tap_col;
  void* h_out = nullptr;  // hipHostMalloc
  size_t h_out_cap = 0;
  void* h_in = nullptr;   // hipHostMalloc: staging copy of a pageable caller frame (the caller's buffer is free again when rip_submit returns)
  size_t h_in_cap = 0;
  void* h_tap[2] = {nullptr, nullptr};  // hipHostMalloc: the debayered / colour taps of the frame, downloaded with the result
  // where this frame's downloads go: the slot's own pinned buffers above, or the page-locked buffers the caller gave rip_submit_to
  void* dst_out = nullptr;
  void* dst_tap[2] = {nullptr, nullptr};
  int gate_device = -1;  // device whose InflightGate queue holds ev_done (set when the frame is enqueued)
  size_t h_tap_cap[2] = {0, 0};
  hipEvent_t ev_up = nullptr, ev_kernels = nullptr, ev_done = nullptr;
  hipEvent_t ev_start = nullptr, ev_dl_start = nullptr;  // RIP_DEBUG_RING only: before the upload / the download (the other three then carry timestamps too)
  uint64_t ticket = 0;
  bool busy = false;  // submitted, not collected yet
  bool held = false;  // collected: the pinned result and the taps stay put until the next collect (or until a submit needs the slot)
  Plan pl;
  bool has_deb = false, has_col = false;  // the taps this frame keeps on the device
  bool dl_deb = false, dl_col = false;    // ... and downloads into h_tap with the result
  static void reserve_pinned(void*& ptr, size_t& cap, size_t bytes) {
    if (bytes <= cap) return;
    if (ptr) HIP_CHECK(hipHostFree(ptr));
    ptr = nullptr;
    cap = 0;
    HIP_CHECK(hipHostMalloc(&ptr, bytes + bytes / 8, hipHostMallocDefault));
    cap = bytes + bytes / 8;
  }
  void reserve_host(size_t bytes) { reserve_pinned(h_out, h_out_cap, bytes); }
  void reserve_host_in(size_t bytes) { reserve_pinned(h_in, h_in_cap, bytes); }
  void release();  // rip_ring.cpp
};

// ---- the constants a handle keeps on the device (rip_constants.cpp): each with its host copy, its device buffers and whatever says
// whether those are current, side by side ----
// undistortion maps (interleaved float2), built lazily
struct MapConst {
  std::vector<float> host;
  DevBuf dev, ckpt;  // ckpt: scratch of the map kernels (row accumulators at every 32nd column)
  bool dirty = true, uploaded = false;
  bool host_valid = false;  // device-built maps are copied to the host only when something on the host asks for them
};
// compiled remap plan (tiled LDS gather), rebuilt when the maps or the source geometry change
struct PlanConst {
  rip::RemapPlan host;
  DevBuf words, tiles, border, counters;
  DevBuf fp;  // the device compiler's footprint (lo, hi per source row pair), read back into host.fp_lo / fp_hi
  bool uploaded = false;
  bool on_device = false;  // compiled by remap_plan_kernel: host.words / tiles / border stay empty
  int n_border = 0;
  // the fast chain kernel's items inside the plan's footprint (rip::chain_footprint_items), uploaded once per (plan, flip)
  DevBuf items;
  int items_flip = -1;  // -1: not built for the current plan
  int items_n = 0;
};
// colour tables
struct TableConst {
  rip::DevTables host;
  DevBuf dev;
  DevBuf lds_image;  // the fused chain's LDS tables as one image (rip::launch_vig_image)
  DevBuf ccc_accum;  // the ccc estimator's accumulator table (rip::ccc_build_scalar_tables): never changes, uploaded once
  bool dirty = true;
};
// vignetting mask plane per geometry (float, rows x cols)
struct VignetteConst {
  std::vector<float> host;
  DevBuf dev;
  int rows = -1, cols = -1;
  bool dirty = true;
};
// ccc: model spectra, filter state and the estimator's resize geometry
struct CccConst {
  rip::CccModel model;
  DevBuf filter_fft, bias_fft, state;
  bool uploaded = false, state_init = false, reset_pending = false, cfg_dirty = true;
  double kf_h = 0.0, kf_r = 1.0;
  DevBuf geom;  // CccGeomLayout, for frames of geom_rows x geom_cols
  int geom_rows = -1, geom_cols = -1;
};
// The ccc estimator's cv::resize(frame, Size(360, 270)) tables (rip::fill_resize_tables) in CccConst::geom: byte offsets of the parts
struct CccGeomLayout {
  static constexpr int W = 360, H = 270;
  static constexpr size_t xofs = 0;                      // int32 [W]
  static constexpr size_t ialpha = xofs + W * 4;         // int16 [2 W]
  static constexpr size_t yofs = ialpha + 2 * W * 2;     // int32 [2 H]
  static constexpr size_t ibeta = yofs + 2 * H * 4;      // int16 [2 H]
  static constexpr size_t bytes = ibeta + 2 * H * 2;
  // cv::resize's switch to the 2 x 2 mean, which the kernel takes by value (CccParams::geom.area_fast)
  static bool area_fast(int rows, int cols) { return rows == 2 * H && cols == 2 * W; }
};
// output stage (rip_set_output_format): the planar formats' 3 x 256 table, rebuilt and uploaded when the format or the normalisation changes
// -- one per output head (rip_set_output_heads), so that alternating heads do not rebuild each other's table
struct OutputTableConst {
  std::vector<uint8_t> host;
  DevBuf dev;
  bool dirty = true;
  int builds = 0;  // how often the table was rebuilt and uploaded (rip_debug_output_head_info)
};
// resize stage (rip_set_output_size): the tables of rip::build_resize_tables or, under the area interpolation,
// rip::build_resize_area_tables, or, under an antialiased filter, rip::build_resize_aa_tables, rebuilt and uploaded when the
// (R, C, H, W, kind of table: the filter, one of four) they were built for changes -- one set per output head
struct ResizeTableConst {
  int builds = 0;  // how often a table set was built and uploaded (rip_debug_output_head_info)
  std::vector<uint8_t> host;
  DevBuf dev;
  int key[5] = {0, 0, 0, 0, 0};
  int area2 = 0;  // build_resize_tables' flag for that key: the 2 x 2 mean replaces the tables
  int whole = 0;  // build_resize_area_tables' flag and scale for that key: whole factors, no table is read
  float scale = 0.f;
  // build_resize_aa_tables' precisions for that key, and its tile height and LDS rows for 1 ([0]) and 3 ([1]) channels
  int aa_xprec = 0, aa_yprec = 0, aa_tile_rows[2] = {0, 0}, aa_lds_rows[2] = {0, 0};
};
// valid-pixel masks (rip_set_rect_mask; PARITY.md "Rect mask"), built by the getters and never by a frame call.  All images are one
// channel with the staging image's layout rule (rows padded to 16 bytes), so every one-channel launch behind F takes them as its source.
// The mask of a frame geometry: the coverage M of the undistortion (rect_mask_kernel), or an all-255 image of F's size for a frame
// that is not undistorted.  `cov` holds M, `bin` its thresholded twin (M == 255) ? 255 : 0, each built when first asked for.
struct MaskBaseConst {
  // what the images were built for: the generation of the maps (und_init counts), whether the frame is undistorted, the size of the
  // image that enters the remap and the size of the mask itself (the maps' size, or F's)
  struct Key {
    uint64_t generation = 0;
    int remap = 0, src_rows = 0, src_cols = 0, rows = 0, cols = 0;
    bool operator==(const Key& o) const {
      return generation == o.generation && remap == o.remap && src_rows == o.src_rows && src_cols == o.src_cols && rows == o.rows && cols == o.cols;
    }
  } key;
  DevBuf cov, bin;
  bool cov_valid = false, bin_valid = false;
  int builds = 0;  // images built since the handle was created (rip_debug_rect_mask_info)
  size_t pitch() const { return pitch16((size_t)key.cols); }
};
// The delivered mask M' of one output head: what the head's window, target, fit mode and filter make of the mask above, under the
// mode it was built for.  One per head, like the table caches; dropped by the head's output setters and by whatever drops M.
struct MaskHeadConst {
  MaskBaseConst::Key base;
  int mode = 0;
  int geom[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // win_x, win_y, win_w, win_h, pic_x, pic_y, pic_w, pic_h, dl_rows, dl_cols, filter kernel
  DevBuf img;
  bool valid = false;
  int builds = 0;  // rip_debug_rect_mask_info
};

}  // namespace rip::api

struct rip_pipeline {
  int device = 0;
  hipStream_t stream = nullptr;
  rip::Modules m;
  // environment overrides, read once when the handle is created (never on a frame path)
  rip::Tunables tn;
  bool maps_on_host = false;      // RIP_MAPS_ON_HOST
  bool plan_on_host = false;      // RIP_PLAN_ON_HOST: compile the remap plan on the host even when the maps are on the device
  std::string debug_dir = "/tmp"; // RIP_DEBUG_DIR
  std::string ccc_model_env;      // RIP_CCC_MODEL
  mutable std::string last_error;
  int tap_mask = RIP_TAP_DEBAYERED | RIP_TAP_COLOR | RIP_TAP_PROCESSED;
  int tap_download_mask = 0;  // rip_set_tap_download: which of the kept taps rip_submit also downloads with the result
  int fp_contract = 0;        // rip_set_fp_contraction / RIP_FP_CONTRACT: contraction model of the float stages (0 none, 1 fused)

  // constants on the device
  rip::api::MapConst maps;
  rip::api::PlanConst plan;
  rip::api::TableConst tables;
  rip::api::VignetteConst vignette;
  rip::api::CccConst ccc;
  rip::api::OutputTableConst out_table[rip::kMaxOutputHeads];   // indexed by output head
  rip::api::ResizeTableConst rsz_tables[rip::kMaxOutputHeads];
  // what the last frame call that delivered head k did for it (rip_debug_output_head_info): the chain wrote it directly -- also
  // true of an identity head of a single-output call -- or head_copy_kernel copied it from the staging image
  struct HeadRecord {
    int direct_write = 0, copied = 0;
  } head_record[rip::kMaxOutputHeads];
  // valid-pixel masks (rip_set_rect_mask): the generation of the maps (und_init counts: everything that rebuilds or replaces them
  // goes through it), the mask of the last geometry asked for, one delivered mask per head, and the geometry of the last frame call
  // -- undistorted or not, and the size of the image that entered its remap -- which is all RIP_IMAGE_RECT_MASK needs of a frame
  uint64_t maps_generation = 1;
  rip::api::MaskBaseConst mask_base;
  rip::api::MaskHeadConst mask_head[rip::kMaxOutputHeads];
  struct MaskFrame {
    bool remap = false;
    int src_rows = 0, src_cols = 0;
  } mask_frame;
  // per-batch scratch.  d_stats.clean_bytes: the prefix known to hold zeroed FrameStats records (the grey-world / pca statistics
  // kernels clean up after themselves).  d_hist.clean_bytes: the leading bytes known to be zero -- the ccc estimator's global-atomic
  // histogram (small batches) hands its counters back zeroed, so a stream of single frames pays for one memset, not one per frame
  rip::api::DevBuf d_stats, d_wb, d_hist, d_work, d_rowbest, d_argmax, d_mid;
  rip::api::DevBuf d_mht;  // the Malvar-He-Cutler image of a batch when no DEBAYERED tap holds it (run_batch)
  // output and resize stage: the pipeline's final image of a batch slice in front of the converter, and the resized image of the slice
  // in front of the converter (only under a format); rows of both padded to 16 bytes
  rip::api::DevBuf d_fmt, d_rsz;
  // the tables of a head's CLAHE (rip_clahe.hpp), n frames x tiles x 256 bytes: written and read inside one call, nothing is kept
  rip::api::DevBuf d_clahe;
  // the format "jpeg" (rip_jpeg.hpp).  Per call: the quantised coefficients of a batch slice, 2 bytes per coded sample, and one word
  // per restart interval and frame -- no stream is staged, the kernels write into the caller's slots.  Per head: the tables and the
  // header blob of the key (quality, restart rows, rows, cols, channels) they were built for, and the stream lengths of the head's
  // last frame call (rip_get_output_jpeg_sizes): jpeg_frames[k] words, 0 after a frame call that delivered another format from head k.
  rip::api::DevBuf d_jpeg_coef, d_jpeg_intervals;
  rip::api::DevBuf d_jpeg_tables[rip::kMaxOutputHeads], d_jpeg_header[rip::kMaxOutputHeads], d_jpeg_sizes[rip::kMaxOutputHeads];
  int jpeg_key[rip::kMaxOutputHeads][5] = {};
  int jpeg_frames[rip::kMaxOutputHeads] = {};
  int last_chain_walked = 0;  // items per frame the last chain launch of run_batch walked (rip_debug_chain_footprint)
  bool use_tiled_remap = true;
  int last_batch_frames = 0;
  bool work_enqueued = false;  // some frame call has put work on `stream` (rip_set_stream orders a new stream behind it)
  // cross-kernel overlap inside one batch (run_batch): the remap of frame group g runs on this internal stream while the
  // statistics and the fused chain of group g + 1 run on the caller's stream
  hipStream_t aux_stream = nullptr;
  std::vector<hipEvent_t> ovl_events;
  hipEvent_t switch_event = nullptr;  // rip_set_stream: orders the new stream behind the work left on the old one
  // asynchronous host path: frames in flight (rip_submit / rip_collect), upload and download streams
  std::vector<std::unique_ptr<rip::api::RingSlot>> ring;
  int ring_depth = 3;
  uint64_t next_ticket = 1;
  hipStream_t ul_stream = nullptr, dl_stream = nullptr;
  // optional per-kernel timing with HIP events on the handle's stream (bench.py roofline leg)
  bool prof_on = false;
  std::vector<hipEvent_t> prof_events;  // pairs
  std::vector<int> prof_ids;
  size_t prof_used = 0;
  // rip_debug_launch_log: which kernels the handle's calls launched
  bool launch_log_on = false;
  rip::LaunchLog launch_log;
  // host-apply staging and last-frame taps
  rip::api::DevBuf d_in, d_out, d_tap_deb, d_tap_col, d_dbg;
  rip::api::DevBuf d_head_out[rip::kMaxOutputHeads];  // rip_apply_heads: the delivered frame of every requested head, tightly packed
  int last_rows[3] = {0, 0, 0}, last_cols[3] = {0, 0, 0}, last_cn[3] = {0, 0, 0};
  bool last_valid[3] = {false, false, false};
  rip::api::DevBuf* last_buf[3] = {nullptr, nullptr, nullptr};
  const void* last_host[3] = {nullptr, nullptr, nullptr};  // pinned host copy of the image (frames that came through rip_collect), else null

  ~rip_pipeline();  // rip_api.cpp
};

namespace rip::api {

// RAII marker: records an event pair around the launches of one kernel class when profiling is on
struct ProfScope {
  rip_pipeline* p;
  hipStream_t stream;  // the stream the class's kernels are launched on (the handle's, or the internal overlap stream)
  size_t slot = (size_t)-1;
  ProfScope(rip_pipeline* pp, int id, hipStream_t s) : p(pp), stream(s) {
    if (!p->prof_on || p->prof_used + 2 > p->prof_events.size()) return;
    slot = p->prof_used;
    p->prof_used += 2;
    p->prof_ids.push_back(id);
    (void)hipEventRecord(p->prof_events[slot], stream);
  }
  ~ProfScope() {
    if (slot != (size_t)-1) (void)hipEventRecord(p->prof_events[slot + 1], stream);
  }
};

// RAII: points this thread's launch-record sink at the handle's log (when that is on) around the code that launches kernels
struct LaunchLogScope {
  rip::LaunchLog* before;
  explicit LaunchLogScope(rip_pipeline* p) : before(rip::t_launch_log) { rip::t_launch_log = p->launch_log_on ? &p->launch_log : nullptr; }
  ~LaunchLogScope() { rip::t_launch_log = before; }
  LaunchLogScope(const LaunchLogScope&) = delete;
  LaunchLogScope& operator=(const LaunchLogScope&) = delete;
};

rip_status status_of(const std::exception& e);  // rip_api.cpp: the status an exception of a C-ABI call stands for
// runs the body of a C-ABI call: an exception becomes the handle's last error and a status
template <typename F>
rip_status guarded(const rip_pipeline* p, F&& fn) {
  try {
    fn();
    return RIP_OK;
  } catch (const std::exception& e) {
    if (p) p->last_error = e.what();
    return status_of(e);
  }
}

// rip_api.cpp
void need(const rip_pipeline* p);         // a handle
void need_device(const rip_pipeline* p);  // ... that has a device
void need_head(const rip_pipeline* p, int head);  // ... and this output head
void copy_string(const std::string& s, char* out, size_t cap);
// what the selected head delivers for such a frame: make_plan + apply_output_format, behind the refusal of a null encoding
Plan delivered_plan(const rip_pipeline* p, int rows, int cols, int channels, const char* encoding);

// rip_plan.cpp: no HIP call
int parse_packed(const std::string& e, int& ry, int& rx);
size_t row_bytes(const Plan& pl, int cols, int channels);
size_t delivered_bytes(const Plan& pl);
Plan make_plan(const rip::Modules& m, int rows, int cols, int channels, const std::string& encoding);
void apply_output_format(const rip::Modules& m, int head, Plan& pl);
FrameView tight_output_view(const Plan& pl, void* d_out);
FrameView resolve_output_layout(const Plan& pl, void* d_out, size_t out_step, size_t out_frame_stride);
// The caller's input frames as a view, the pitches resolved (0: tightly packed) and refused in this order: a row pitch smaller than
// a row -- resolve_input_pitches, for the frame call that has refusals of its own to place behind this one -- then a frame stride
// smaller than a frame, then a pitch or a frame too large.
void resolve_input_pitches(const Plan& pl, int rows, int cols, int channels, size_t& in_step, size_t& in_frame_stride);
ConstFrameView resolve_input_layout(const Plan& pl, const void* d_in, size_t in_step, size_t in_frame_stride, int rows, int cols, int channels);

// rip_constants.cpp: the device-resident constants, each rebuilt and uploaded when what it was built from has changed
void und_init(rip_pipeline* p);
void ensure_host_maps(rip_pipeline* p);
void need_host_map(rip_pipeline* p);
void ensure_maps(rip_pipeline* p);
void ensure_plan(rip_pipeline* p, int src_rows, int src_cols);
int ensure_chain_items(rip_pipeline* p, int rows, int cols, int flip_angle);
void ensure_tables(rip_pipeline* p);
void ensure_vignette(rip_pipeline* p, int rows, int cols);
void ensure_ccc(rip_pipeline* p, int rows, int cols);
void ensure_output_table(rip_pipeline* p, int head, int fmt);
// the tables and the header of a head's JPEG streams for the plan's picture and settings (d_jpeg_tables, d_jpeg_header)
void ensure_jpeg_constants(rip_pipeline* p, const Plan& pl);
// The resize stage's tables of head `head` for an R x C window and an H x W picture, written into the table fields of the launch's
// parameter block `r` -- device pointers into ResizeTableConst::dev and the flags that go with them; the other fields are left alone.
void ensure_resize_tables(rip_pipeline* p, int head, int R, int C, int H, int W, rip::ResizeParams& r);
void ensure_area_tables(rip_pipeline* p, int head, int R, int C, int H, int W, rip::AreaParams& r);
// filter: 2 (linear_aa) or 3 (cubic_aa), rip::output_interpolation_id's numbers; channels: 1 or 3, picks tile_rows and lds_rows
void ensure_aa_tables(rip_pipeline* p, int head, int filter, int channels, int R, int C, int H, int W, rip::AaParams& r);
// What a setting invalidates, said once: the loaders and setters (rip_settings.cpp) call these and und_init and write no flag
// themselves.  invalidate_head: the delivered mask of output head `head` and, with `table`, its output table (the resize tables
// are keyed, not flagged); invalidate_all_heads: both of every head.
void invalidate_head(rip_pipeline* p, int head, bool table);
void invalidate_all_heads(rip_pipeline* p);
void invalidate_color_tables(rip_pipeline* p);  // gamma and the Lab / HSV tables (ensure_tables)
void invalidate_vignette(rip_pipeline* p);      // the mask plane (ensure_vignette)
void invalidate_ccc_config(rip_pipeline* p);    // the estimator's configuration (ensure_ccc)
void invalidate_ccc_model(rip_pipeline* p);     // the model spectra on the device
void restart_ccc_estimator(rip_pipeline* p);    // first frame, new Kalman filter

// rip_batch.cpp: the chain (run_batch) and write_debug_dumps.  rip_output_stage.cpp: everything else down to the end of this
// namespace -- what follows the chain: resize, pad, converter, heads and masks
size_t fmt_pitch(const Plan& pl);
void run_batch(rip_pipeline* p, const Plan& pl, ConstFrameView src, FrameView dst, Taps taps, int n, bool reuse_wb = false);
// first_frame (here and in run_batch_heads): the index of the slice's first frame inside the frame call
void run_batch_formatted(rip_pipeline* p, const Plan& pl, ConstFrameView src, FrameView dst, Taps taps, int n, int first_frame = 0);
// A frame call of n_frames frames begins, behind its last refusal: a head that delivers "jpeg" gets room for its stream lengths
// (rip_get_output_jpeg_sizes), which the slices of the call fill from their first_frame on; any other head's count goes to 0.
void begin_jpeg_call(rip_pipeline* p, const Plan& pl, int n_frames);
// rip_apply / rip_apply_heads: waits for the stream, then copies the stream of a one-frame jpeg head from the device slot `d_slot`
// to `out` -- the length first, then the used bytes only
void download_jpeg_frame(rip_pipeline* p, const Plan& pl, const void* d_slot, uint8_t* out);
// Several delivered images from one run of the chain (rip_apply_device_heads): plans[k] / dsts[k] for every head k < n_heads, with
// dsts[k].ptr null for a head that is not requested (its plan is not looked at).  pl: make_plan's, the pipeline's own image.
void run_batch_heads(rip_pipeline* p, const Plan& pl, const Plan* plans, const FrameView* dsts, int n_heads, ConstFrameView src, Taps taps, int n, int first_frame = 0);
// the heads calls' checks behind make_plan (rip.h rip_apply_device_heads, steps 5 to 7): fills plans[k] and views[k] of every
// requested head (requested[k]; the others are neither planned nor validated); view_of(k, plan) resolves head k's buffer with its
// own refusals.  The messages of step 5 are prefixed "output head <k>: " and keep their status.  Nothing is enqueued here.
template <typename ViewOf>
void plan_heads(const rip::Modules& m, const Plan& pl, int n_heads, const bool* requested, bool any_tap, Plan* plans, FrameView* views, ViewOf&& view_of) {
  int n_requested = 0;
  for (int k = 0; k < n_heads; k++) {
    views[k] = FrameView{nullptr, 0, 0, 0, 0};
    if (!requested[k]) continue;
    n_requested++;
    const std::string prefix = "output head " + std::to_string(k) + ": ";
    try {
      plans[k] = pl;
      apply_output_format(m, k, plans[k]);
      views[k] = view_of(k, plans[k]);
    } catch (const AssertError& e) {
      throw AssertError(prefix + e.what());
    } catch (const CapacityError& e) {
      throw CapacityError(prefix + e.what());
    } catch (const std::invalid_argument& e) {
      throw InvalidArgument(prefix + e.what());
    }
  }
  if (pl.out_elem_bytes == 2 && n_requested > 1)
    throw InvalidArgument("16-bit Bayer frames without a 16-bit range give bgr16, which one output head at a time can deliver; " + std::to_string(n_requested) + " were requested");
  if (pl.out_elem_bytes == 2 && any_tap) throw InvalidArgument("16-bit Bayer frames have no taps");
}
void write_debug_dumps(rip_pipeline* p, const Plan& pl, ConstFrameView src, const uint8_t* final_image);
// Valid-pixel masks (rip_set_rect_mask; PARITY.md "Rect mask").  What a frame call leaves for RIP_IMAGE_RECT_MASK: two ints and a flag
inline void remember_mask_frame(rip_pipeline* p, const Plan& pl) { p->mask_frame = {pl.remap, pl.mid_rows, pl.mid_cols}; }
// The mask of a frame geometry on the device, built on the handle's stream unless it is cached: the coverage M of the current maps
// for a src_rows x src_cols image entering the remap (remap; rows x cols is then the maps' size), else all 255 of rows x cols;
// binary: its thresholded twin.  Rows are pitch() bytes apart.
ConstFrameView ensure_mask_base(rip_pipeline* p, bool remap, int src_rows, int src_cols, int rows, int cols, bool binary);
// The delivered mask of head pl.head for the frame of `pl` (make_plan + apply_output_format of that frame) under mode 1 (coverage) or
// 2 (valid): dl_rows x dl_cols, one channel, cached per head.
ConstFrameView ensure_mask_head(rip_pipeline* p, const Plan& pl, int mode);

}  // namespace rip::api
