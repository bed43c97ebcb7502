// rip_batch.cpp -- from a Plan to the kernels: the route a batch takes through the kernels of rip_chain/stats/ccc/remap/fused/
// demosaic.hip (enqueue_*, plan_route, run_chain, run_batch) and the debug dumps; the output stage behind it is rip_output_stage.cpp.
// The device-resident constants a batch needs come from rip_constants.cpp.  Everything is enqueued on the handle's stream.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rip_handle.hpp"

namespace rip::api {

namespace {

// where a kernel reads its frames: the five source fields every parameter block of rip_kernels.hpp starts with
template <typename Params>
void set_source(Params& d, ConstFrameView src) {
  d.src = src.ptr;
  d.src_step = src.step;
  d.src_frame_stride = src.frame_stride;
  d.rows = src.rows;
  d.cols = src.cols;
}

// The stand-alone demosaic kernels' common parameters (Raw16Params, MhtParams, Debayer16Params)
template <typename Params>
Params demosaic_params(const Plan& pl, ConstFrameView src, FrameView out, int n) {
  Params d = {};
  set_source(d, src);
  d.bayer_ry = pl.ry;
  d.bayer_rx = pl.rx;
  d.dst = out.ptr;
  d.dst_step = out.step;
  d.dst_frame_stride = out.frame_stride;
  d.flip_angle = pl.flip_angle;
  d.n_frames = n;
  return d;
}

// Malvar-He-Cutler demosaic (rip_set_debayer_method "mht", rip_demosaic.hip): one pass of its own writes the post-flip BGR
// image -- the DEBAYERED tap (flip.cpp:60-62), into the caller's tap buffer when one was requested, else into d_mht -- and the
// rest of the chain runs on that image exactly as on a bgr8 frame holding it, with no flip left to do.
// 16-bit frames with a range (rip_set_debayer_16bit_range, rip_raw16.hip) and packed frames (rip_packed.hip) take the same
// route with either method: demosaic at 16 bits + narrowing + flip in one pass, into the same destination.
// 16-bit frames without a range (one kernel, no taps, either method): the pass writes the bgr16 result into the caller's
// output and that is all.  Returns false then -- the batch is complete -- and otherwise true with the image it wrote in `bgr`.
bool enqueue_demosaic_pass(rip_pipeline* p, const Plan& pl, ConstFrameView src, FrameView dst, Taps taps, int n, ConstFrameView& bgr) {
  const bool bgr16 = pl.out_elem_bytes == 2;
  FrameView out = dst;
  if (!bgr16) {
    // tight when it is the tap; else 16-byte aligned rows and frames: what launch_remap_tiled asks of the image it gathers from
    const size_t step = taps.debayered ? (size_t)pl.mid_cols * 3 : ((size_t)pl.mid_cols * 3 + 15) & ~(size_t)15;
    out = {taps.debayered, step, step * pl.mid_rows, pl.mid_rows, pl.mid_cols};
    if (!out.ptr) {
      p->d_mht.reserve(out.frame_stride * (size_t)n);
      out.ptr = p->d_mht.as<uint8_t>();
    }
  }
  {
    ProfScope ps(p, RIP_KERNEL_CHAIN, p->stream);
    if (pl.raw16) {
      rip::Raw16Params d = demosaic_params<rip::Raw16Params>(pl, src, out, n);
      d.mht = pl.mht ? 1 : 0;
      d.black = pl.black;
      d.white = pl.white;
      if (pl.packed_layout) rip::launch_packed(d, pl.packed_layout, p->stream);
      else rip::launch_raw16(d, p->stream);
    } else if (pl.mht) {
      rip::MhtParams d = demosaic_params<rip::MhtParams>(pl, src, out, n);
      d.elem_bytes = pl.in_elem_bytes;
      d.drows = pl.mid_rows;
      d.dcols = pl.mid_cols;
      rip::launch_demosaic_mht(d, p->stream);
    } else {  // 16-bit Bayer extension with the range off, bilinear
      rip::Debayer16Params d = demosaic_params<rip::Debayer16Params>(pl, src, out, n);
      d.drows = pl.out_rows;
      d.dcols = pl.out_cols;
      rip::launch_debayer16(d, p->stream);
    }
  }
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) throw DeviceError(std::string("kernel launch failed: ") + hipGetErrorString(le));
  if (bgr16) p->last_batch_frames = 0;  // no white balance ran: rip_get_white_balance_info must not hand out an earlier batch's gains
  bgr = out;
  return !bgr16;
}

// the plan of the frames enqueue_demosaic_pass wrote: plain bgr8, already flipped (their DEBAYERED tap is written too)
Plan as_bgr8_after_demosaic(const Plan& pl) {
  Plan s = pl;
  s.raw16 = s.mht = false;
  s.in_elem_bytes = 1;
  s.packed_layout = 0;
  s.src_kind = rip::SRC_BGR;
  s.ry = s.rx = 0;
  s.flip_angle = 0;
  return s;
}

// Which kernels a batch goes through: decided once by plan_route, before the first launch, and executed by run_chain
struct BatchRoute {
  enum Remap {
    NONE,         // no undistortion: the chain writes the caller's output
    FUSED_BAYER,  // chain + remap in one kernel that reads the Bayer frames (rip_fused.hip)
    DIRECT,       // no chain: the remap gathers from the caller's frames as they lie
    DIRECT_MONO,  // ... and the ring kernel flips by 180 degrees and applies the gamma table as it gathers
    AFTER_CHAIN   // the chain writes chain_dst, the remap gathers from it
  } remap = NONE;
  bool tiled = false;     // the plan is compiled and the tiled / ring kernel is tried first
  bool no_tap = true;     // neither tap requested
  FrameView chain_dst{};  // the caller's output, the COLOR tap, or d_mid (16-byte pitch)
  int chain_items = -1;   // -1 dense, else the footprint list's length
  int groups = 1, per_group = 0;  // overlap_groups split (1 = off)
  hipStream_t back = nullptr;     // the remap's stream: the handle's internal one with groups > 1, else the caller's
};

// white-balance methods estimated from per-frame sums (FrameStats)
bool wb_from_sums(const Plan& pl) { return pl.wb_mode == rip::WB_Q8 || pl.wb_mode == rip::WB_PCA || pl.wb_mode == rip::WB_SIMPLE; }

// the remap's view of ng frames: plan, destination (frames f0.. of dst), and -- `src` -- either the intermediate image or, on
// the fused and direct routes, the caller's frames themselves
rip::RemapTiledParams remap_params(const rip_pipeline* p, const Plan& pl, ConstFrameView src, FrameView dst, int f0, int ng) {
  rip::RemapTiledParams tp = {};
  rip::RemapParams& r = tp.base;
  set_source(r, src);
  r.channels = pl.channels;
  r.map_xy = p->maps.dev.as<float>();
  r.dst = dst.ptr + (size_t)f0 * dst.frame_stride;
  r.dst_step = dst.step;
  r.dst_frame_stride = dst.frame_stride;
  r.drows = pl.out_rows;
  r.dcols = pl.out_cols;
  r.n_frames = ng;
  tp.words = p->plan.words.as<uint32_t>();
  tp.tiles = p->plan.tiles.as<rip::RemapTileDesc>();
  tp.tiles_x = p->plan.host.tiles_x;
  tp.tiles_y = p->plan.host.tiles_y;
  tp.border_list = p->plan.border.as<uint32_t>();
  tp.n_border = p->plan.n_border;
  tp.lds_bytes = (unsigned)p->plan.host.max_lds_bytes;
  return tp;
}
// DIRECT_MONO: the chain's two operations, done by the ring kernel
rip::RemapTiledParams mono_ops(const rip_pipeline* p, const Plan& pl, rip::RemapTiledParams tp) {
  tp.mono_lut = (pl.stage_bits & rip::ST_GAMMA) ? p->tables.dev.as<uint8_t>() + offsetof(rip::DevTables, gamma_lut) : nullptr;
  tp.mono_flip180 = pl.flip_angle == 180 ? 1 : 0;
  return tp;
}
// the chain's parameters for ng frames (dst / taps filled in by the caller)
rip::ChainParams chain_params(const rip_pipeline* p, const Plan& pl, ConstFrameView src, rip::FrameWb* wb, int ng) {
  rip::ChainParams c = {};
  set_source(c, src);
  c.src_kind = pl.src_kind;
  c.bayer_ry = pl.ry;
  c.bayer_rx = pl.rx;
  c.drows = pl.mid_rows;
  c.dcols = pl.mid_cols;
  c.channels = pl.channels;
  c.flip_angle = pl.flip_angle;
  c.n_frames = ng;
  c.wb_mode = pl.wb_mode;
  c.wb = wb;
  c.stage_bits = pl.stage_bits;
  for (int i = 0; i < 9; i++) c.cc_m[i] = p->m.cc_matrix[i];
  for (int i = 0; i < 3; i++) c.cc_bias[i] = (float)p->m.cc_bias[i];
  if (pl.stage_bits & rip::ST_VIG) c.vig_mask = p->vignette.dev.as<float>();
  // cv::Scalar(hue_gain_, saturation_gain_, value_gain_) on (H,S,V), color_enhancer.cpp:42
  c.hsv_gain[0] = (float)p->m.ce_hue_gain;
  c.hsv_gain[1] = (float)p->m.ce_saturation_gain;
  c.hsv_gain[2] = (float)p->m.ce_value_gain;
  c.tabs = p->tables.dev.as<rip::DevTables>();
  c.vig_image = p->tables.lds_image.as<uint32_t>();
  c.fp_contract = p->fp_contract;
  return c;
}

// Everything that allocates, uploads or synchronises happens here, before the first launch of the chain; the two dry runs ask
// the fused and the ring kernel whether they take the geometry.
BatchRoute plan_route(rip_pipeline* p, const Plan& pl, ConstFrameView src, FrameView dst, Taps taps, int n, bool reuse_wb) {
  BatchRoute rt;
  rt.no_tap = !taps.color && !taps.debayered;
  rt.chain_dst = dst;
  p->d_wb.reserve(sizeof(rip::FrameWb) * (size_t)n);
  if (reuse_wb) {
    if (p->last_batch_frames != n) throw DeviceError("internal: white-balance gains of another batch");
  } else if (wb_from_sums(pl)) {
    p->d_stats.reserve(sizeof(rip::FrameStats) * (size_t)n);
    if (pl.wb_mode == rip::WB_SIMPLE) p->d_hist.reserve((size_t)n * 768 * sizeof(unsigned));
  } else if (pl.wb_mode == rip::WB_FLOAT) {
    ensure_ccc(p, pl.mid_rows, pl.mid_cols);
    p->d_hist.reserve((size_t)n * rip::ccc_hist_split(n) * 65536 * sizeof(unsigned));
    p->d_work.reserve((size_t)n * 65536 * 2 * sizeof(float));
    p->d_rowbest.reserve((size_t)n * 256 * 2 * sizeof(float));
    p->d_argmax.reserve((size_t)n * 2 * sizeof(int));
  }
  if (pl.remap) {
    ensure_maps(p);
    if (p->use_tiled_remap && (pl.channels == 3 || pl.channels == 1)) {
      ensure_plan(p, pl.mid_rows, pl.mid_cols);
      rt.tiled = true;
    }
    rt.remap = BatchRoute::AFTER_CHAIN;
    // Memory-rate stage sets with neither tap requested: the remap's tiles demosaic and colour their own source rectangles
    // out of the Bayer frames (rip_fused.hip) -- no intermediate image is written, read or even allocated.
    if (rt.tiled && rt.no_tap && pl.src_kind == rip::SRC_BAYER &&
        rip::launch_remap_fused(remap_params(p, pl, src, dst, 0, n), chain_params(p, pl, src, p->d_wb.as<rip::FrameWb>(), n), p->plan.host.max_rect_w,
                                p->plan.host.max_rect_h, p->tn, p->stream, /*dry_run=*/true))
      rt.remap = BatchRoute::FUSED_BAYER;
    // bgr8 / mono8 frames with nothing to do before the undistortion (no flip, no white balance, no stage, no tap): the
    // chain would be a copy -- the remap gathers from the caller's frames as they lie
    else if (rt.no_tap && (pl.src_kind == rip::SRC_BGR || pl.src_kind == rip::SRC_MONO) && pl.flip_angle == 0 && pl.wb_mode == rip::WB_NONE &&
             pl.stage_bits == 0)
      rt.remap = BatchRoute::DIRECT;
    // mono8: the whole chain is a 180-degree flip and the gamma table -- the ring kernel addresses the mirrored rectangle
    // and maps the taps through the table as it gathers them
    else if (rt.tiled && rt.no_tap && pl.src_kind == rip::SRC_MONO && (pl.flip_angle == 0 || pl.flip_angle == 180) && p->tn.remap_fused &&
             rip::launch_remap_tiled(mono_ops(p, pl, remap_params(p, pl, src, dst, 0, n)), p->tn, p->stream, /*dry_run=*/true))
      rt.remap = BatchRoute::DIRECT_MONO;
    // The pre-undistortion image: tightly packed when it is an API output (the COLOR tap: written once, gathered from), else
    // internal with 16-byte aligned rows (the tiled remap stages it with aligned 16-byte loads)
    const size_t tap_pitch = (size_t)pl.mid_cols * pl.channels;
    const size_t mid_pitch = taps.color ? tap_pitch : ((tap_pitch + 15) & ~(size_t)15);
    rt.chain_dst = {taps.color, mid_pitch, mid_pitch * pl.mid_rows, pl.mid_rows, pl.mid_cols};
    if (rt.remap == BatchRoute::AFTER_CHAIN && !taps.color) {
      p->d_mid.reserve(rt.chain_dst.frame_stride * (size_t)n);
      rt.chain_dst.ptr = p->d_mid.as<uint8_t>();
    }
  }
  // In front of the remap, with no tap asking for the whole intermediate image, the fast Bayer kernel computes only the items
  // whose pixels the remap reads (its plan's footprint: the corners a fisheye map never samples are ~21 % of config 2's frame).
  // The statistics pass above it still reads every pixel: the white-balance estimates are defined over the whole frame.
  const int rows = src.rows, cols = src.cols;
  if (rt.tiled && rt.remap == BatchRoute::AFTER_CHAIN && rt.no_tap && p->tn.chain_footprint && pl.src_kind == rip::SRC_BAYER && pl.channels == 3 &&
      (pl.flip_angle == 0 || pl.flip_angle == 180) && rows % 2 == 0 && cols % 4 == 0 && rows / 2 <= 65535 && cols / 4 <= 65535 &&
      rows == pl.mid_rows && cols == pl.mid_cols && p->plan.host.fp_lo.size() == (size_t)(rows + 1) / 2)
    rt.chain_items = ensure_chain_items(p, rows, cols, pl.flip_angle);
  if (pl.stage_bits & rip::ST_VIG) ensure_vignette(p, pl.mid_rows, pl.mid_cols);
  // Frame groups (tunable overlap_groups > 1; OFF by default): with the batch cut into G groups of frames, remap(g) runs on the
  // handle's internal stream beside stats(g + 1) and chain(g + 1) on the caller's stream (overlap_mode 1), or beside stats(g + 1)
  // only (mode 2: the chain waits for the remap).  raw_image_pipeline.hpp:143-172 only orders the stages of ONE frame, and
  // everything that carries state from frame to frame -- the ccc Kalman filter -- stays on the caller's stream in frame order;
  // the caller's stream waits for the internal one before run_chain returns, so the batch is complete in stream order
  // exactly as without the split.  Measured on config2 (256 frames, one box, round 3): 4.87 ms per step unsplit; mode 1 with
  // 2 / 4 / 8 / 16 groups 4.98 / 5.00 / 5.09 / 5.70; mode 2 with 2 / 4 groups 4.94 / 5.05 -- the three kernels lean on the
  // same VALU issue slots and LDS, and the shorter launches pay their tails (docs/experiments_r1-3.md), so the default stays 1.
  if (pl.remap && !reuse_wb && p->tn.overlap_groups > 1) rt.groups = std::min(p->tn.overlap_groups, n);
  rt.back = p->stream;
  if (rt.groups > 1) {
    if (!p->aux_stream) HIP_CHECK(hipStreamCreateWithFlags(&p->aux_stream, hipStreamNonBlocking));
    while (p->ovl_events.size() < 2 * (size_t)rt.groups + 1) {
      hipEvent_t e;
      HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      p->ovl_events.push_back(e);
    }
    rt.back = p->aux_stream;
  }
  rt.per_group = (n + rt.groups - 1) / rt.groups;
  return rt;
}

// The white-balance estimate of frames f0 .. f0 + ng of a batch of n: statistics and finalisation, gains into d_wb[f0..].
// stats_clean_before: the prefix of d_stats known to be zero when the batch began.
void enqueue_wb_estimate(rip_pipeline* p, const Plan& pl, const BatchRoute& rt, ConstFrameView src, int f0, int ng, int n, size_t stats_clean_before) {
  const hipStream_t front = p->stream;
  rip::FrameWb* wb_g = p->d_wb.as<rip::FrameWb>() + f0;
  if (wb_from_sums(pl)) {
    rip::FrameStats* stats_g = p->d_stats.as<rip::FrameStats>() + f0;
    unsigned* hist_g = pl.wb_mode == rip::WB_SIMPLE ? p->d_hist.as<unsigned>() + (size_t)f0 * 768 : nullptr;
    if (hist_g) p->d_hist.clean_bytes = 0;  // the same buffer serves SimpleWB's histograms
    // grey-world / pca: the statistics kernel itself finishes a frame (gains written by the workgroup that ends last) and
    // hands its FrameStats back zeroed, so neither a memset nor a finalisation launch separates the batches -- two
    // dependent launches less on the single-frame path.  The records are cleared here only when they are not known to be
    // clean: fresh memory, or a batch that did not run to its end.
    const bool fused_finalize = pl.wb_mode != rip::WB_SIMPLE;
    const size_t stats_bytes = sizeof(rip::FrameStats) * (size_t)n;
    if (!fused_finalize || stats_clean_before < stats_bytes) HIP_CHECK(hipMemsetAsync(stats_g, 0, sizeof(rip::FrameStats) * (size_t)ng, front));
    p->d_stats.clean_bytes = 0;  // until this batch has been enqueued completely
    if (hist_g) HIP_CHECK(hipMemsetAsync(hist_g, 0, (size_t)ng * 768 * sizeof(unsigned), front));
    rip::StatsParams sp = {};
    set_source(sp, src);
    sp.src_kind = pl.src_kind;
    sp.bayer_ry = pl.ry;
    sp.bayer_rx = pl.rx;
    sp.n_frames = ng;
    sp.mode = pl.wb_mode;
    sp.thresh255 = (unsigned)(uint16_t)std::lrintf((float)p->m.wb_bright_thr * 255);
    sp.stats = stats_g;
    sp.hist3 = hist_g;
    sp.wb_out = fused_finalize ? wb_g : nullptr;
    {
      ProfScope ps(p, RIP_KERNEL_STATS, front);
      rip::launch_stats(sp, p->tn, front);
    }
    // SimpleWB::setP(clipping_percentile_) (white_balance.cpp:55); total = pixels per channel plane
    if (!fused_finalize)
      rip::launch_wb_finalize(pl.wb_mode, sp.stats, nullptr, nullptr, p->tables.dev.as<rip::DevTables>(), wb_g, ng, front, sp.hist3,
                              (float)p->m.wb_percentile, src.rows * src.cols);
  } else if (pl.wb_mode == rip::WB_FLOAT) {
    rip::CccParams cp = {};  // the launcher zeroes the histogram when its kernel accumulates in HBM
    set_source(cp, src);
    cp.src_kind = pl.src_kind;
    cp.bayer_ry = pl.ry;
    cp.bayer_rx = pl.rx;
    cp.flip_angle = pl.flip_angle;
    cp.drows = pl.mid_rows;
    cp.dcols = pl.mid_cols;
    cp.n_frames = ng;
    const uint8_t* gm = p->ccc.geom.as<uint8_t>();
    cp.geom.xofs = reinterpret_cast<const int*>(gm + CccGeomLayout::xofs);
    cp.geom.ialpha = reinterpret_cast<const short*>(gm + CccGeomLayout::ialpha);
    cp.geom.yofs = reinterpret_cast<const int*>(gm + CccGeomLayout::yofs);
    cp.geom.ibeta = reinterpret_cast<const short*>(gm + CccGeomLayout::ibeta);
    cp.geom.area_fast = CccGeomLayout::area_fast(pl.mid_rows, pl.mid_cols) ? 1 : 0;
    // setSaturationThreshold(float, float): thresholds are held as float (:437-440); 255 * thr in float
    cp.upper = 255 * (float)p->m.wb_bright_thr;
    cp.lower = 255 * (float)p->m.wb_dark_thr;
    cp.hist_split = rip::ccc_hist_split(n);  // of the whole batch: what d_hist was sized for
    cp.hist_counts = p->d_hist.as<unsigned>() + (size_t)f0 * cp.hist_split * 65536;
    cp.accum_tab = p->tables.ccc_accum.as<float>();
    cp.work = p->d_work.as<float>() + (size_t)f0 * 65536 * 2;
    cp.filter_fft = p->ccc.filter_fft.as<float>();
    cp.bias_fft = p->ccc.bias_fft.as<float>();
    cp.row_best = p->d_rowbest.as<float>() + (size_t)f0 * 256 * 2;
    cp.argmax = p->d_argmax.as<int>() + (size_t)f0 * 2;
    cp.tabs = p->tables.dev.as<rip::DevTables>();
    const size_t hist_bytes = (size_t)ng * 65536 * sizeof(unsigned);  // what the global-atomic kernel accumulates into
    cp.hist_is_clean = (rt.groups == 1 && p->d_hist.clean_bytes >= hist_bytes) ? 1 : 0;
    p->d_hist.clean_bytes = 0;  // until the estimator has been enqueued completely
    bool estimated;
    int left_clean = 0;
    {
      ProfScope ps(p, RIP_KERNEL_CCC, front);
      estimated = rip::launch_ccc_estimate(cp, p->tn, front, &left_clean);
    }
    // no histogram, no estimate: fail before the finalisation advances the persistent Kalman state on stale data
    if (!estimated) throw DeviceError("ccc white balance: a kernel of the estimator could not be launched");
    if (left_clean && rt.groups == 1) p->d_hist.clean_bytes = hist_bytes;
    const bool inline_argmax = rip::ccc_argmax_in_finalize(ng);
    rip::launch_wb_finalize(rip::WB_FLOAT, nullptr, cp.argmax, p->ccc.state.as<rip::CccState>(), cp.tabs, wb_g, ng, front, nullptr, 0.f, 0,
                            inline_argmax ? cp.row_best : nullptr, inline_argmax ? cp.argmax : nullptr);
  }
}

// FUSED_BAYER: chain + remap of group g in one kernel (memory-rate stage sets, no taps)
void enqueue_fused_remap(rip_pipeline* p, const Plan& pl, ConstFrameView src, FrameView dst, int f0, int ng, int n) {
  ProfScope ps(p, RIP_KERNEL_REMAP, p->stream);
  rip::ChainParams fc = chain_params(p, pl, src, p->d_wb.as<rip::FrameWb>() + f0, ng);
  fc.dst_streaming = (n >= 8 && p->tn.chain_nt != 0) ? 1 : 0;  // the kernel's output is the batch's final image: non-temporal stores for batches
  if (!rip::launch_remap_fused(remap_params(p, pl, src, dst, f0, ng), fc, p->plan.host.max_rect_w, p->plan.host.max_rect_h, p->tn, p->stream, /*dry_run=*/false))
    throw DeviceError("internal: the fused remap refused a geometry it had accepted");
}

// The fused chain of group g (frames f0 .. f0 + ng of n) into the route's chain_dst, the DEBAYERED tap beside it
void enqueue_chain(rip_pipeline* p, const Plan& pl, const BatchRoute& rt, ConstFrameView src, FrameView dst, Taps taps, int g, int f0, int ng, int n) {
  const hipStream_t front = p->stream;
  const size_t tap_pitch = (size_t)pl.mid_cols * pl.channels, tap_frame = tap_pitch * pl.mid_rows;  // taps are tightly packed API outputs
  rip::ChainParams c = chain_params(p, pl, src, p->d_wb.as<rip::FrameWb>() + f0, ng);
  c.dst = rt.chain_dst.ptr + (size_t)f0 * rt.chain_dst.frame_stride;
  c.dst_step = rt.chain_dst.step;
  c.dst_frame_stride = rt.chain_dst.frame_stride;
  // Non-temporal stores for batches: the image is far larger than the L2s, so lines the chain leaves there only get in the
  // way.  Rounds 3-4 kept them for images no kernel of the batch reads again (debayer-only, 256 frames: 1.08 against 1.16
  // ms; the remap of that time lost 19 % behind them); with the LDS-DMA ring remap it is the other way round (round 5, config 2:
  // remap 1.94-1.97 -> 1.83-1.85 ms behind a chain that stores non-temporally) -- tunable chain_nt
  c.dst_streaming = (n >= 8 && p->tn.chain_nt != 0 && (!pl.remap || p->tn.chain_nt < 0)) ? 1 : 0;
  c.tap = taps.debayered ? taps.debayered + (size_t)f0 * tap_frame : nullptr;
  c.tap_frame_stride = tap_frame;
  c.deal = pl.remap ? -1 : 0;  // hint for launch_chain: the remap gathers from this image next (Tunables::chain_deal)
  if (rt.chain_items >= 0 && rip::chain_uses_fast_path(c)) {
    c.item_list = p->plan.items.as<uint32_t>();
    c.n_list_items = rt.chain_items;
  }
  p->last_chain_walked = c.item_list ? rt.chain_items : (src.rows / 2) * (src.cols / 4);
  // overlap_mode 2: only the statistics of this group share the chip with the remap of the previous one; the chain waits
  if (rt.back != front && p->tn.overlap_mode == 2 && g > 0) HIP_CHECK(hipStreamWaitEvent(front, p->ovl_events[rt.groups + g - 1], 0));
  {
    ProfScope ps(p, RIP_KERNEL_CHAIN, front);
    rip::launch_chain(c, p->tn, front);
  }
  if (!pl.remap && taps.color) {
    // pre-undistortion copy == final image when no remap follows
    for (int f = f0; f < f0 + ng; f++)
      HIP_CHECK(hipMemcpy2DAsync(taps.color + (size_t)f * tap_frame, tap_pitch, dst.ptr + (size_t)f * dst.frame_stride, dst.step, tap_pitch,
                                 (size_t)pl.mid_rows, hipMemcpyDeviceToDevice, front));
  }
}

// The undistortion of one group on `stream`: the tiled / ring kernel where the route has a compiled plan and the kernel takes
// the geometry, else the plain gather.  DIRECT_MONO has no second choice: the plain gather neither flips nor applies the table.
void enqueue_remap(rip_pipeline* p, const BatchRoute& rt, const rip::RemapTiledParams& tp, hipStream_t stream) {
  bool done = false;
  if (rt.tiled) {
    ProfScope ps(p, RIP_KERNEL_REMAP, stream);
    done = rip::launch_remap_tiled(tp, p->tn, stream);
  }
  if (!done && rt.remap == BatchRoute::DIRECT_MONO) throw DeviceError("internal: the ring remap refused a geometry it had accepted");
  if (!done) {
    ProfScope ps(p, RIP_KERNEL_REMAP, stream);
    if (!rip::launch_remap(tp.base, stream)) throw InvalidArgument("undistortion: frame geometry exceeds the kernels' 32-bit addressing");
  }
}

// The chain on 8-bit frames, from the white-balance estimate to the undistorted image
void run_chain(rip_pipeline* p, const Plan& pl, ConstFrameView src, FrameView dst, Taps taps, int n, bool reuse_wb) {
  ensure_tables(p);
  const BatchRoute rt = plan_route(p, pl, src, dst, taps, n, reuse_wb);
  const size_t stats_clean_before = p->d_stats.clean_bytes;  // behind plan_route's reserve: 0 when that grew the buffer
  const hipStream_t front = p->stream, back = rt.back;
  const int groups = rt.groups;
  // Whatever was enqueued on the internal stream is joined into the caller's stream when this function is left -- also by
  // an exception: the batch is complete, in the caller's stream order, once the last remap is.
  struct Join {
    rip_pipeline* p;
    int slot;
    bool used = false;
    ~Join() {
      if (!used) return;
      (void)hipEventRecord(p->ovl_events[slot], p->aux_stream);
      (void)hipStreamWaitEvent(p->stream, p->ovl_events[slot], 0);
    }
  } join{p, 2 * groups};
  for (int g = 0; g < groups; g++) {
    const int f0 = g * rt.per_group, ng = std::min(rt.per_group, n - f0);
    if (ng <= 0) break;
    const ConstFrameView src_g = frames_from(src, f0);
    if (!reuse_wb) enqueue_wb_estimate(p, pl, rt, src_g, f0, ng, n, stats_clean_before);
    if (rt.remap == BatchRoute::FUSED_BAYER) {
      enqueue_fused_remap(p, pl, src_g, dst, f0, ng, n);
    } else if (rt.remap == BatchRoute::DIRECT) {  // no chain at all: the remap reads the input frames
      enqueue_remap(p, rt, remap_params(p, pl, src_g, dst, f0, ng), front);
    } else if (rt.remap == BatchRoute::DIRECT_MONO) {
      enqueue_remap(p, rt, mono_ops(p, pl, remap_params(p, pl, src_g, dst, f0, ng)), front);
    } else {
      enqueue_chain(p, pl, rt, src_g, dst, taps, g, f0, ng, n);
      if (rt.remap == BatchRoute::NONE) continue;
      if (back != front) {  // remap(g) starts when chain(g) is done; the caller's stream goes on with group g + 1
        HIP_CHECK(hipEventRecord(p->ovl_events[g], front));
        HIP_CHECK(hipStreamWaitEvent(back, p->ovl_events[g], 0));
        join.used = true;
      }
      enqueue_remap(p, rt, remap_params(p, pl, frames_from(ConstFrameView(rt.chain_dst), f0), dst, f0, ng), back);
      if (back != front && p->tn.overlap_mode == 2) HIP_CHECK(hipEventRecord(p->ovl_events[groups + g], back));
    }
  }
  p->last_batch_frames = n;
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) throw DeviceError(std::string("kernel launch failed: ") + hipGetErrorString(le));
  if (wb_from_sums(pl) && !reuse_wb && pl.wb_mode != rip::WB_SIMPLE)  // every statistics launch went out: its records come back zeroed
    p->d_stats.clean_bytes = std::max(stats_clean_before, sizeof(rip::FrameStats) * (size_t)n);
}

}  // namespace

// Enqueues the whole chain for n frames of `src` into `dst`; either tap may be null.
// reuse_wb: the white-balance gains of the previous launch (same frames) are applied again and no estimator runs -- the
// debug stage dumps re-run prefixes of the chain without advancing the ccc Kalman state.
void run_batch(rip_pipeline* p, const Plan& pl, ConstFrameView src, FrameView dst, Taps taps, int n, bool reuse_wb) {
  p->work_enqueued = true;  // from here on something may sit on p->stream
  DeviceGuard device_guard(p->device);
  LaunchLogScope log_scope(p);
  if (!pl.raw16 && !pl.mht && pl.out_elem_bytes == 1) {  // the chain demosaics by itself (bilinear, 8 bits)
    run_chain(p, pl, src, dst, taps, n, reuse_wb);
    return;
  }
  ConstFrameView bgr;
  if (enqueue_demosaic_pass(p, pl, src, dst, taps, n, bgr)) run_chain(p, as_bgr8_after_demosaic(pl), bgr, dst, {nullptr, taps.color}, n, reuse_wb);
}

// setDebug(true): raw_image_pipeline.hpp:143-172 writes the image after EVERY module -- enabled or not -- to
// /tmp/0N_<module>.png through saveDebugImage (:179-186: copy, cv::normalize(0, 255, NORM_MINMAX), cv::imwrite).  The modules
// are one fused kernel here, so the image after module k is produced by running the chain once more with the modules after k
// switched off (same input frame still on the device: src; same white-balance gains: reuse_wb).  RIP_DEBUG_DIR replaces /tmp.
void write_debug_dumps(rip_pipeline* p, const Plan& pl, ConstFrameView src, const uint8_t* final_image) {
  static const char* const kNames[8] = {"00_debayer", "01_flip", "02_white_balancing", "03_color_calibration", "04_gamma_correction",
                                        "05_vignetting_correction", "06_color_enhancer", "07_undistortion"};
  static const int kStages[8] = {0, 0, 0, rip::ST_CC, rip::ST_CC | rip::ST_GAMMA, rip::ST_CC | rip::ST_GAMMA | rip::ST_VIG,
                                 rip::ST_CC | rip::ST_GAMMA | rip::ST_VIG | rip::ST_HSV, rip::ST_CC | rip::ST_GAMMA | rip::ST_VIG | rip::ST_HSV};
  const std::string& dir = p->debug_dir;
  std::vector<uint8_t> host;
  // the re-runs below are not launches of the caller's frame: keep them out of an active rip_profile_begin/end session
  // (they would skew its per-class averages and use up its event slots), and out of the launch record (rip_debug_launch_log)
  struct ProfPause {
    rip_pipeline* p;
    bool was, log_was;
    explicit ProfPause(rip_pipeline* pp) : p(pp), was(pp->prof_on), log_was(pp->launch_log_on) { p->prof_on = p->launch_log_on = false; }
    ~ProfPause() {
      p->prof_on = was;
      p->launch_log_on = log_was;
    }
  } prof_pause(p);
  std::string failed;
  for (int k = 0; k < 8; k++) {
    int r, c;
    if (k == 7) {  // after the undistortion module: the output of this call
      r = pl.out_rows;
      c = pl.out_cols;
      host.assign(final_image, final_image + (size_t)r * c * pl.channels);
    } else {
      Plan s = pl;
      s.remap = false;
      if (k < 1) s.flip_angle = 0;
      const bool swap = s.flip_angle == 90 || s.flip_angle == 270;
      s.mid_rows = swap ? src.cols : src.rows;
      s.mid_cols = swap ? src.rows : src.cols;
      if (k < 2) s.wb_mode = rip::WB_NONE;
      s.stage_bits &= kStages[k];
      s.out_rows = r = s.mid_rows;
      s.out_cols = c = s.mid_cols;
      const size_t bytes = (size_t)r * c * s.channels;
      p->d_dbg.reserve(bytes);
      run_batch(p, s, src, {p->d_dbg.as<uint8_t>(), (size_t)c * s.channels, bytes, r, c}, {nullptr, nullptr}, 1, /*reuse_wb=*/true);
      host.resize(bytes);
      HIP_CHECK(hipMemcpyAsync(host.data(), p->d_dbg.ptr, bytes, hipMemcpyDeviceToHost, p->stream));
      HIP_CHECK(hipStreamSynchronize(p->stream));
    }
    rip::normalize_minmax_u8(host.data(), host.size());
    const std::string path = dir + "/" + kNames[k] + ".png";
    if (!rip::write_png(path, host.data(), r, c, pl.channels)) {
      std::fprintf(stderr, "raw_image_pipeline: could not write %s\n", path.c_str());
      failed += (failed.empty() ? "" : ", ") + path;
    }
  }
  // cv::imwrite's failure does not fail apply() in the reference either; the message stays readable through rip_last_error()
  if (!failed.empty()) p->last_error = "debug dumps not written: " + failed;
}

}  // namespace rip::api
