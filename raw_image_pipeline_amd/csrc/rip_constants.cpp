// rip_constants.cpp -- the device-resident constants a batch needs (rip_handle.hpp: maps, remap plan and item list, colour tables,
// vignetting mask, ccc model, output table, resize tables).  Every ensure_* returns at once when its constant is current; else it
// rebuilds the host copy, uploads it on the handle's stream and waits for that stream before its host staging goes away.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rip_handle.hpp"

namespace rip::api {

// `bytes` of host memory into a buffer of at least max(bytes, min_cap), on the handle's stream.  Does not wait: the caller
// synchronises once, behind its last copy.
static void upload(rip_pipeline* p, DevBuf& buf, const void* host, size_t bytes, size_t min_cap = 0) {
  buf.reserve(std::max(bytes, min_cap));
  if (bytes) HIP_CHECK(hipMemcpyAsync(buf.ptr, host, bytes, hipMemcpyHostToDevice, p->stream));
}

// ------------------------------------------------------------------------------------------------
// undistortion bookkeeping: UndistortionModule::init() (undistortion.cpp:197-238) minus the map
// generation, which is deferred until a frame (or rip_init_undistortion) needs it.
// ------------------------------------------------------------------------------------------------
void und_init(rip_pipeline* p) {
  rip::Modules& m = p->m;
  double newK[9];
  if (rip::is_pinhole_model(m.dist_model)) {
    // plumb_bob / radtan / rational_polynomial: cv::getOptimalNewCameraMatrix with alpha = balance (not in the reference)
    double k[8];
    rip::pinhole_coefficients(m.dist_model, m.dist_D, k);
    rip::pinhole_estimate_new_camera_matrix(m.dist_K, k, m.dist_w, m.dist_h, m.balance, m.rect_w, m.rect_h, m.fov_scale, newK);
  } else {
    rip::fisheye_estimate_new_camera_matrix(m.dist_K, m.dist_D, m.dist_w, m.dist_h, m.dist_R, m.balance, m.rect_w, m.rect_h,
                                            m.fov_scale, newK);
  }
  std::memcpy(m.rect_K, newK, sizeof(newK));
  for (int i = 0; i < 8; i++) m.rect_D[i] = 0;
  const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  std::memcpy(m.rect_R, eye, sizeof(eye));
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) m.rect_P[i * 4 + j] = m.rect_K[i * 3 + j];
  p->maps.dirty = true;
  p->maps_generation++;  // the masks built from the maps before this call are no longer current (MaskBaseConst::Key)
}

// ------------------------------------------------------------------------------------------------
// what a setting invalidates (rip_settings.cpp): the flags the ensure_* functions below look at, set here and nowhere else
// ------------------------------------------------------------------------------------------------
void invalidate_head(rip_pipeline* p, int head, bool table) {
  p->mask_head[head].valid = false;
  if (table) p->out_table[head].dirty = true;
}
void invalidate_all_heads(rip_pipeline* p) {
  for (int k = 0; k < rip::kMaxOutputHeads; k++) invalidate_head(p, k, true);
}
void invalidate_color_tables(rip_pipeline* p) { p->tables.dirty = true; }
void invalidate_vignette(rip_pipeline* p) { p->vignette.dirty = true; }
void invalidate_ccc_config(rip_pipeline* p) { p->ccc.cfg_dirty = true; }
void invalidate_ccc_model(rip_pipeline* p) { p->ccc.uploaded = false; }
void restart_ccc_estimator(rip_pipeline* p) { p->ccc.state_init = false; }

// Where the maps are built: on the device for device handles (rip_maps.hip: one thread per map row, FP64, double-double
// atan -- milliseconds instead of 0.25-0.5 s of host threads per calibration change), on the host for RIP_DEVICE_NONE handles
// and when RIP_MAPS_ON_HOST is set (A/B and debugging).  Both produce the same floats (tests/test_parity_gpu.py).
static bool maps_on_device(const rip_pipeline* p) { return p->device != RIP_DEVICE_NONE && !p->maps_on_host; }

void ensure_host_maps(rip_pipeline* p) {
  MapConst& mp = p->maps;
  if (!mp.dirty) return;
  const rip::Modules& m = p->m;
  if (m.dist_w <= 0 || m.dist_h <= 0) throw AssertError("undistortion: image size is not set");
  const size_t n = (size_t)m.dist_w * m.dist_h * 2;
  mp.host.resize(n);
  // maps have the *dist* image size even after setNewImageSize (undistortion.cpp:216)
  const bool pinhole = rip::is_pinhole_model(m.dist_model);  // every other name builds fisheye maps, as the reference does
  if (maps_on_device(p)) {
    DeviceGuard device_guard(p->device);
    LaunchLogScope log_scope(p);
    rip::UndistortMapParams fp = {};
    std::memcpy(fp.K, m.dist_K, sizeof(fp.K));
    fp.pinhole = pinhole ? 1 : 0;
    if (pinhole)
      rip::pinhole_coefficients(m.dist_model, m.dist_D, fp.D);
    else
      std::memcpy(fp.D, m.dist_D, 4 * sizeof(double));
    rip::fisheye_inverse_PR(m.rect_K, m.dist_R, fp.iR);
    fp.w = m.dist_w;
    fp.h = m.dist_h;
    mp.dev.reserve(n * sizeof(float));
    fp.map_xy = mp.dev.as<float>();
    mp.ckpt.reserve(rip::undistort_ckpt_bytes(fp.w, fp.h));
    fp.ckpt = mp.ckpt.as<double>();
    rip::launch_undistort_maps(fp, p->stream);
    // no host copy yet: the remap-plan compiler runs on the device too; need_host_map() fetches the floats for
    // rip_get_undistortion_maps or for a plan compiled on the host
    mp.dirty = false;
    mp.uploaded = true;
    mp.host_valid = false;
    p->plan.host.valid = false;
    return;
  }
  if (pinhole) {
    double k[8];
    rip::pinhole_coefficients(m.dist_model, m.dist_D, k);
    rip::pinhole_init_undistort_rectify_map(m.dist_K, k, m.dist_R, m.rect_K, m.dist_w, m.dist_h, mp.host.data());
  } else {
    rip::fisheye_init_undistort_rectify_map(m.dist_K, m.dist_D, m.dist_R, m.rect_K, m.dist_w, m.dist_h, mp.host.data());
  }
  mp.dirty = false;
  mp.uploaded = false;
  mp.host_valid = true;
  p->plan.host.valid = false;
}

// the maps as floats on the host
void need_host_map(rip_pipeline* p) {
  ensure_host_maps(p);
  MapConst& mp = p->maps;
  if (mp.host_valid) return;
  DeviceGuard device_guard(p->device);
  HIP_CHECK(hipMemcpyAsync(mp.host.data(), mp.dev.ptr, mp.host.size() * sizeof(float), hipMemcpyDeviceToHost, p->stream));
  HIP_CHECK(hipStreamSynchronize(p->stream));
  mp.host_valid = true;
}

void ensure_maps(rip_pipeline* p) {
  ensure_host_maps(p);
  MapConst& mp = p->maps;
  if (mp.uploaded) return;
  upload(p, mp.dev, mp.host.data(), mp.host.size() * sizeof(float));
  HIP_CHECK(hipStreamSynchronize(p->stream));
  mp.uploaded = true;
}

static_assert(rip::kRemapOutside == rip::kPlanOutside && rip::kRemapBorder == rip::kPlanBorder, "plan sentinels");
static_assert(sizeof(rip::RemapTile) == sizeof(rip::RemapTileDesc), "tile descriptor layout");

void ensure_plan(rip_pipeline* p, int src_rows, int src_cols) {
  ensure_maps(p);
  LaunchLogScope log_scope(p);
  const rip::Modules& m = p->m;
  PlanConst& c = p->plan;
  rip::RemapPlan& pl = c.host;
  if (!pl.valid || pl.src_rows != src_rows || pl.src_cols != src_cols || pl.drows != m.dist_h || pl.dcols != m.dist_w) {
    c.on_device = false;
    c.items_flip = -1;
    if (maps_on_device(p) && !p->plan_on_host) {
      // Compile the plan where the maps are (rip_maps.hip remap_plan_kernel: one workgroup per tile; the same words, tile
      // rectangles and border pixels as rip::compile_remap_plan, the border list in another order): no 8 B/px map read-back,
      // no 4 B/px plan upload, no host threads -- a calibration change costs the map kernel plus ~0.1 ms.
      pl = rip::RemapPlan();
      pl.drows = m.dist_h;
      pl.dcols = m.dist_w;
      pl.src_rows = src_rows;
      pl.src_cols = src_cols;
      pl.tiles_x = (pl.dcols + rip::kRemapTileW - 1) / rip::kRemapTileW;
      pl.tiles_y = (pl.drows + rip::kRemapTileH - 1) / rip::kRemapTileH;
      const size_t ntiles = (size_t)pl.tiles_x * pl.tiles_y;
      const unsigned border_cap = 1u << 20;  // pixels; more than that (a map that mostly straddles the border) goes to the host
      c.words.reserve(ntiles * rip::kRemapTilePx * sizeof(uint32_t));
      c.tiles.reserve(ntiles * sizeof(rip::RemapTileDesc));
      c.border.reserve((size_t)border_cap * sizeof(uint32_t));
      c.counters.reserve(4 * sizeof(unsigned));
      HIP_CHECK(hipMemsetAsync(c.counters.ptr, 0, 4 * sizeof(unsigned), p->stream));
      rip::RemapPlanBuildParams bp = {};
      bp.map_xy = p->maps.dev.as<float>();
      bp.drows = pl.drows;
      bp.dcols = pl.dcols;
      bp.src_rows = src_rows;
      bp.src_cols = src_cols;
      bp.tiles_x = pl.tiles_x;
      bp.tiles_y = pl.tiles_y;
      bp.words = c.words.as<uint32_t>();
      bp.tiles = c.tiles.as<rip::RemapTileDesc>();
      bp.border = c.border.as<uint32_t>();
      bp.border_cap = border_cap;
      bp.counters = c.counters.as<unsigned>();
      rip::launch_remap_plan_build(bp, p->stream);
      // the footprint of the same quantised taps (rip::compile_remap_footprint's hull): lo starts at 0x7F7F7F7F, hi at 0
      const int pairs = (src_rows + 1) / 2;
      c.fp.reserve(2 * (size_t)pairs * sizeof(int));
      HIP_CHECK(hipMemsetAsync(c.fp.ptr, 0x7F, (size_t)pairs * sizeof(int), p->stream));
      HIP_CHECK(hipMemsetAsync(c.fp.as<int>() + pairs, 0, (size_t)pairs * sizeof(int), p->stream));
      rip::RemapFootprintParams fq = {};
      fq.map_xy = bp.map_xy;
      fq.drows = pl.drows;
      fq.dcols = pl.dcols;
      fq.src_rows = src_rows;
      fq.src_cols = src_cols;
      fq.tiles_x = pl.tiles_x;
      fq.tiles_y = pl.tiles_y;
      fq.lo = c.fp.as<int>();
      fq.hi = c.fp.as<int>() + pairs;
      rip::launch_remap_footprint(fq, p->stream);
      pl.fp_lo.resize(pairs);
      pl.fp_hi.resize(pairs);
      unsigned counters[4] = {0, 0, 0, 0};
      HIP_CHECK(hipMemcpyAsync(counters, c.counters.ptr, sizeof(counters), hipMemcpyDeviceToHost, p->stream));
      HIP_CHECK(hipMemcpyAsync(pl.fp_lo.data(), fq.lo, (size_t)pairs * sizeof(int), hipMemcpyDeviceToHost, p->stream));
      HIP_CHECK(hipMemcpyAsync(pl.fp_hi.data(), fq.hi, (size_t)pairs * sizeof(int), hipMemcpyDeviceToHost, p->stream));
      HIP_CHECK(hipStreamSynchronize(p->stream));
      for (int i = 0; i < pairs; i++)
        if (pl.fp_lo[i] >= pl.fp_hi[i]) pl.fp_lo[i] = INT32_MAX, pl.fp_hi[i] = 0;  // the host compiler's "no tap" form
      if (counters[0] <= border_cap) {
        c.n_border = (int)counters[0];
        pl.max_lds_bytes = counters[1];
        pl.max_rect_w = (int)counters[2];
        pl.max_rect_h = (int)counters[3];
        pl.valid = true;
        c.on_device = true;
        c.uploaded = true;
      }
    }
    if (!c.on_device) {
      need_host_map(p);
      rip::compile_remap_plan(pl, p->maps.host.data(), m.dist_h, m.dist_w, src_rows, src_cols);
      c.n_border = (int)pl.border.size();
      c.uploaded = false;
    }
  }
  if (!c.uploaded) {
    upload(p, c.words, pl.words.data(), pl.words.size() * sizeof(uint32_t));
    upload(p, c.tiles, pl.tiles.data(), pl.tiles.size() * sizeof(rip::RemapTile));
    upload(p, c.border, pl.border.data(), pl.border.size() * sizeof(uint32_t), 4);
    HIP_CHECK(hipStreamSynchronize(p->stream));
    c.uploaded = true;
  }
}

// The fast chain kernel's items whose output the remap reads (rip::chain_footprint_items on the current plan's footprint), on
// the device; uploaded once per (plan, flip).  Returns how many there are, or -1 when the footprint covers more than 95 % of
// the frame (balance 1, wide fields of view): the dense walk is as good there and needs no table.
int ensure_chain_items(rip_pipeline* p, int rows, int cols, int flip_angle) {
  PlanConst& c = p->plan;
  if (c.items_flip != flip_angle) {
    std::vector<uint32_t> items;
    rip::chain_footprint_items(c.host.fp_lo, c.host.fp_hi, rows, cols, flip_angle, items);
    const long long dense = (long long)(rows / 2) * (cols / 4);
    c.items_n = (long long)items.size() * 20 > dense * 19 ? -1 : (int)items.size();
    if (c.items_n >= 0) {
      upload(p, c.items, items.data(), items.size() * sizeof(uint32_t), 4);
      HIP_CHECK(hipStreamSynchronize(p->stream));
    }
    c.items_flip = flip_angle;
  }
  return c.items_n;
}

void ensure_tables(rip_pipeline* p) {
  TableConst& tc = p->tables;
  if (!tc.dirty) return;
  LaunchLogScope log_scope(p);
  rip::DevTables& t = tc.host;
  const rip::ColorTables& c = rip::color_tables();
  rip::build_gamma_lut(p->m.gamma_k, t.gamma_lut);
  for (int i = 0; i < 256; i++) t.lin_tab[i] = c.srgb_gamma[p->m.gamma_enabled ? t.gamma_lut[i] : i];
  std::memcpy(t.cbrt_tab, c.cbrt, sizeof(t.cbrt_tab));
  for (int i = 0; i < 256; i++) t.yf_tab[i] = (uint32_t)c.lab_to_yf[2 * i] | ((uint32_t)c.lab_to_yf[2 * i + 1] << 16);
  for (int i = 0; i < 4096; i++) t.inv_gamma[i] = (uint8_t)std::min<int>(255, c.inv_gamma[i]);
  std::memcpy(t.sdiv, c.sdiv, sizeof(t.sdiv));
  std::memcpy(t.hdiv, c.hdiv180, sizeof(t.hdiv));
  std::memcpy(t.lab_fwd, c.fwd, sizeof(t.lab_fwd));
  std::memcpy(t.lab_inv, c.inv, sizeof(t.lab_inv));
  for (int ch = 0; ch < 3; ch++) {
    if (c.inv[ch * 3] < -32768 || c.inv[ch * 3] > 32767 || c.inv[ch * 3 + 1] < -32768 || c.inv[ch * 3 + 1] > 32767)
      throw std::runtime_error("Lab inverse coefficients do not fit 16 bits");
    t.lab_inv_pk[ch * 2] = (int32_t)(((uint32_t)c.inv[ch * 3] & 0xffffu) | ((uint32_t)c.inv[ch * 3 + 1] << 16));
    t.lab_inv_pk[ch * 2 + 1] = c.inv[ch * 3 + 2];
  }
  std::vector<float> accum;
  rip::ccc_build_scalar_tables(t.log_tab, accum, t.exp_neg_tab);
  rip::fft256_twiddles(t.tw_re, t.tw_im);
  upload(p, tc.dev, &t, sizeof(t));
  tc.lds_image.reserve(rip::vig_image_bytes());
  rip::launch_vig_image(tc.dev.as<rip::DevTables>(), tc.lds_image.as<uint32_t>(), p->stream);
  if (!tc.ccc_accum.ptr) upload(p, tc.ccc_accum, accum.data(), accum.size() * sizeof(float));
  HIP_CHECK(hipStreamSynchronize(p->stream));  // host staging buffers go out of scope
  tc.dirty = false;
}

void ensure_vignette(rip_pipeline* p, int rows, int cols) {
  VignetteConst& v = p->vignette;
  if (!v.dirty && v.rows == rows && v.cols == cols) return;
  rip::build_vignette_mask(rows, cols, p->m.vig_scale, p->m.vig_a2, p->m.vig_a4, v.host, p->fp_contract);
  upload(p, v.dev, v.host.data(), v.host.size() * sizeof(float));
  HIP_CHECK(hipStreamSynchronize(p->stream));
  v.rows = rows;
  v.cols = cols;
  v.dirty = false;
}

void ensure_ccc(rip_pipeline* p, int rows, int cols) {
  CccConst& c = p->ccc;
  if (!c.model.loaded) {
    if (!p->ccc_model_env.empty()) {
      if (!rip::ccc_load_model_file(c.model, p->ccc_model_env)) throw InvalidArgument("RIP_CCC_MODEL: cannot read " + p->ccc_model_env);
      c.uploaded = false;
    } else {
      throw InvalidArgument(
          "white balance method [ccc] needs a model: call rip_load_ccc_model()/rip_set_ccc_model() or set RIP_CCC_MODEL "
          "(the reference loads raw_image_pipeline_white_balance/model/default.bin)");
    }
  }
  if (!c.uploaded) {
    const size_t bytes = 65536 * 2 * sizeof(float);
    upload(p, c.filter_fft, c.model.filter_fft.data(), bytes);
    upload(p, c.bias_fft, c.model.bias_fft.data(), bytes);
    HIP_CHECK(hipStreamSynchronize(p->stream));
    c.uploaded = true;
  }
  if (!c.state_init) {
    rip::CccState s = {};
    s.first_frame = 1;
    s.uv_x = s.uv_y = 128;  // uv_pos_ = (height/2, width/2), :178
    s.st_x = s.st_y = 128.f;
    s.kf_h = (float)c.kf_h;
    s.kf_r = (float)c.kf_r;
    s.temporal = p->m.wb_temporal ? 1 : 0;
    upload(p, c.state, &s, sizeof(s));
    HIP_CHECK(hipStreamSynchronize(p->stream));
    c.state_init = true;
    c.reset_pending = false;
    c.cfg_dirty = false;
  }
  if (c.reset_pending || c.cfg_dirty) {
    // patch individual fields, stream-ordered, keeping the filter state
    rip::CccState* d = c.state.as<rip::CccState>();
    if (c.reset_pending) {
      static const int one = 1;
      HIP_CHECK(hipMemcpyAsync(&d->first_frame, &one, sizeof(int), hipMemcpyHostToDevice, p->stream));
    }
    float hr[2] = {(float)c.kf_h, (float)c.kf_r};
    int temporal = p->m.wb_temporal ? 1 : 0;
    HIP_CHECK(hipMemcpyAsync(&d->kf_h, hr, sizeof(hr), hipMemcpyHostToDevice, p->stream));
    HIP_CHECK(hipMemcpyAsync(&d->temporal, &temporal, sizeof(int), hipMemcpyHostToDevice, p->stream));
    HIP_CHECK(hipStreamSynchronize(p->stream));
    c.reset_pending = false;
    c.cfg_dirty = false;
  }
  if (c.geom_rows != rows || c.geom_cols != cols) {
    // cv::resize(src, small, Size(360, 270)) coefficient tables (imgproc/resize.cpp), for frames of any size
    using L = CccGeomLayout;
    alignas(4) uint8_t raw[L::bytes];
    rip::fill_resize_tables(rows, cols, L::H, L::W, reinterpret_cast<int32_t*>(raw + L::xofs), reinterpret_cast<int16_t*>(raw + L::ialpha),
                            reinterpret_cast<int32_t*>(raw + L::yofs), reinterpret_cast<int16_t*>(raw + L::ibeta));
    upload(p, c.geom, raw, L::bytes);
    HIP_CHECK(hipStreamSynchronize(p->stream));
    c.geom_rows = rows;
    c.geom_cols = cols;
  }
}

// The planar formats' table on the device, rebuilt on the host (rip::build_output_table) when the format or the normalisation
// has changed since the last frame
void ensure_output_table(rip_pipeline* p, int head, int fmt) {
  OutputTableConst& t = p->out_table[head];
  if (!t.dirty) return;
  const rip::OutputHead& h = p->m.heads[head];
  t.builds++;
  t.host.resize(768 * (size_t)rip::output_format_elem_bytes(fmt));
  rip::build_output_table(fmt, h.out_divisor, h.out_mean, h.out_std, t.host.data());
  upload(p, t.dev, t.host.data(), t.host.size(), 768 * 4);
  HIP_CHECK(hipStreamSynchronize(p->stream));
  t.dirty = false;
}

// The tables and the header blob of a head's JPEG streams (rip_jpeg.hpp), rebuilt and uploaded when the key -- quality, restart rows and
// the picture's rows, cols and channels -- is not the one they were built for.
void ensure_jpeg_constants(rip_pipeline* p, const Plan& pl) {
  const int key[5] = {pl.jpeg_quality, pl.jpeg_restart_rows, pl.img_rows, pl.dl_pic_cols, pl.channels};
  int* have = p->jpeg_key[pl.head];
  if (std::memcmp(key, have, sizeof(key)) == 0 && p->d_jpeg_tables[pl.head].ptr) return;
  rip::JpegTables tables;
  uint8_t q[128], header[rip::kJpegHeaderColour];
  rip::jpeg_build_tables(pl.jpeg_quality, tables, q);
  const int n = rip::jpeg_build_header(pl.img_rows, pl.dl_pic_cols, pl.channels, pl.jpeg_restart_rows, q, header);
  upload(p, p->d_jpeg_tables[pl.head], &tables, sizeof(tables));
  upload(p, p->d_jpeg_header[pl.head], header, (size_t)n, rip::kJpegHeaderColour);
  HIP_CHECK(hipStreamSynchronize(p->stream));
  std::memcpy(have, key, sizeof(key));
}

// One table set of the resize stage is kept per output head, whichever filter built it: rebuilt by fill(host copy of `bytes` zeroed bytes)
// and uploaded when the key -- (R, C, H, W, kind of table) -- is not the one it was built for.  The upload goes through the handle's
// pageable copy and waits for the stream, like the other ensure_* functions: a handle that alternates between targets pays that
// wait on every change.
template <typename Fill>
static void ensure_keyed_tables(rip_pipeline* p, int head, const int (&key)[5], size_t bytes, Fill&& fill) {
  ResizeTableConst& t = p->rsz_tables[head];
  if (std::memcmp(key, t.key, sizeof(key)) == 0 && t.dev.ptr) return;
  t.builds++;
  t.host.assign(bytes, 0);
  fill(t.host.data());
  upload(p, t.dev, t.host.data(), bytes);
  HIP_CHECK(hipStreamSynchronize(p->stream));
  std::memcpy(t.key, key, sizeof(key));
}

// The linear tables (rip::build_resize_tables).  One buffer: xofs, alpha (both padded to whole lanes), yofs, beta -- every part starts
// 16-byte aligned.
void ensure_resize_tables(rip_pipeline* p, int head, int R, int C, int H, int W, rip::ResizeParams& r) {
  const size_t wp = rip::resize_table_cols(W), hp = ((size_t)H + 3) & ~(size_t)3;
  const size_t o_alpha = wp * 4, o_yofs = o_alpha + wp * 4, o_beta = o_yofs + hp * 8, bytes = o_beta + hp * 4;
  ensure_keyed_tables(p, head, {R, C, H, W, 0}, bytes, [&](uint8_t* h) {
    rip::build_resize_tables(R, C, H, W, reinterpret_cast<int32_t*>(h), reinterpret_cast<int16_t*>(h + o_alpha), reinterpret_cast<int32_t*>(h + o_yofs),
                             reinterpret_cast<int16_t*>(h + o_beta), &p->rsz_tables[head].area2);
  });
  const uint8_t* d = p->rsz_tables[head].dev.as<uint8_t>();
  r.xofs = reinterpret_cast<const int32_t*>(d);
  r.alpha = reinterpret_cast<const int16_t*>(d + o_alpha);
  r.yofs = reinterpret_cast<const int32_t*>(d + o_yofs);
  r.beta = reinterpret_cast<const int16_t*>(d + o_beta);
  r.area2 = p->rsz_tables[head].area2;
}

// the six index tables AreaParams and AaParams (P) share: xfirst, xcount, xwofs [W] at d, yfirst, ycount, ywofs [H] at d + o_y
template <typename P>
static void set_tap_lists(P& r, const int32_t* d, size_t o_y, int H, int W) {
  r.xfirst = d;
  r.xcount = d + W;
  r.xwofs = d + 2 * (size_t)W;
  r.yfirst = d + o_y;
  r.ycount = d + o_y + H;
  r.ywofs = d + o_y + 2 * (size_t)H;
}

// The tables of the area interpolation (rip::build_resize_area_tables) in the same buffer and under the same key, told apart by the
// key's last entry.  Parts, all of 4-byte entries: xfirst, xcount, xwofs [W], yfirst, ycount, ywofs [H], xweight [C + 2 W],
// yweight [R + 2 H]; wofs is the running sum of count.
void ensure_area_tables(rip_pipeline* p, int head, int R, int C, int H, int W, rip::AreaParams& r) {
  const size_t o_y = (size_t)W * 3, o_xw = o_y + (size_t)H * 3, o_yw = o_xw + (size_t)C + 2 * (size_t)W, words = o_yw + (size_t)R + 2 * (size_t)H;
  ensure_keyed_tables(p, head, {R, C, H, W, 1}, words * 4, [&](uint8_t* bytes) {
    int32_t* h = reinterpret_cast<int32_t*>(bytes);
    rip::build_resize_area_tables(R, C, H, W, h, h + W, reinterpret_cast<float*>(h + o_xw), h + o_y, h + o_y + H, reinterpret_cast<float*>(h + o_yw),
                                  &p->rsz_tables[head].whole, &p->rsz_tables[head].scale);
    for (int axis = 0; axis < 2; axis++) {
      const int d = axis ? H : W;
      const int32_t* count = h + (axis ? o_y : 0) + d;
      int32_t* wofs = h + (axis ? o_y : 0) + 2 * (size_t)d;
      int32_t run = 0;
      for (int i = 0; i < d; i++) {
        wofs[i] = run;
        run += count[i];
      }
    }
  });
  const int32_t* d = p->rsz_tables[head].dev.as<int32_t>();
  set_tap_lists(r, d, o_y, H, W);
  r.xweight = reinterpret_cast<const float*>(d + o_xw);
  r.yweight = reinterpret_cast<const float*>(d + o_yw);
  r.whole = p->rsz_tables[head].whole;
  r.scale = p->rsz_tables[head].scale;
}

// The tables of an antialiased filter (rip::build_resize_aa_tables) in the same buffer and under the same key, whose last entry is
// the filter.  Parts: xfirst, xcount, xwofs [W], yfirst, ycount, ywofs [H] of 4-byte entries, then the int16 weights of the columns
// and of the rows, each part of its capacity rounded up to an even count.
void ensure_aa_tables(rip_pipeline* p, int head, int filter, int channels, int R, int C, int H, int W, rip::AaParams& r) {
  const size_t o_y = (size_t)W * 3, o_xw = o_y + (size_t)H * 3;  // in 4-byte entries
  const size_t cap_x = (rip::resize_aa_weight_capacity(filter, C, W) + 1) & ~(size_t)1, cap_y = (rip::resize_aa_weight_capacity(filter, R, H) + 1) & ~(size_t)1;
  const size_t bytes = o_xw * 4 + (cap_x + cap_y) * 2;
  ResizeTableConst& t = p->rsz_tables[head];
  ensure_keyed_tables(p, head, {R, C, H, W, filter}, bytes, [&](uint8_t* raw) {
    int32_t* h = reinterpret_cast<int32_t*>(raw);
    int16_t* wts = reinterpret_cast<int16_t*>(raw + o_xw * 4);
    rip::build_resize_aa_tables(filter, R, C, H, W, h, h + W, h + 2 * (size_t)W, wts, &t.aa_xprec, h + o_y, h + o_y + H, h + o_y + 2 * (size_t)H, wts + cap_x,
                                &t.aa_yprec, t.aa_tile_rows, t.aa_lds_rows);
  });
  const int32_t* d = t.dev.as<int32_t>();
  const int16_t* dw = reinterpret_cast<const int16_t*>(d + o_xw);
  set_tap_lists(r, d, o_y, H, W);
  r.xweight = dw;
  r.yweight = dw + cap_x;
  r.xprec = t.aa_xprec;
  r.yprec = t.aa_yprec;
  r.tile_rows = t.aa_tile_rows[channels == 3];
  r.lds_rows = t.aa_lds_rows[channels == 3];
}

}  // namespace rip::api
