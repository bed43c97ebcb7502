// rip_ring.cpp -- the frame calls that take and return HOST images: rip_apply (synchronous), rip_submit / rip_submit_to /
// rip_collect (a ring of frames in flight: upload, kernels and download of neighbouring frames overlap), the pinned-memory
// helpers and the image getters.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <mutex>
#include <thread>

#include <pthread.h>

#include "rip_handle.hpp"

namespace rip::api {
namespace {

// Host-side copies of whole frames (the deep copies the reference's API promises: process() and every image getter return a
// clone, raw_image_pipeline.cpp:182-236): a 15 MB memcpy out of the pinned result buffer into freshly allocated pages takes
// 0.4-0.7 ms on one thread -- more than the frame's kernels and its PCIe transfer together -- so copies of 4 MB and more are
// split over a few worker threads (page faults of a fresh destination included).  The pool is created on first use, leaked on
// purpose (its threads may outlive static destruction) and serves one copy at a time; a second caller copies on its own thread.
class CopyPool {
 public:
  static CopyPool& get() {
    static CopyPool* pool = new CopyPool();
    return *pool;
  }
  void copy(void* dst, const void* src, size_t bytes) {
    // a forked child has none of the worker threads and may have inherited the mutexes locked: plain memcpy there
    if (bytes < (size_t(4) << 20) || workers_ == 0 || forked().load(std::memory_order_relaxed) || !busy_.try_lock()) {
      std::memcpy(dst, src, bytes);
      return;
    }
    std::lock_guard<std::mutex> whole(busy_, std::adopt_lock);
    std::unique_lock<std::mutex> lk(mu_);
    dst_ = static_cast<uint8_t*>(dst);
    src_ = static_cast<const uint8_t*>(src);
    bytes_ = bytes;
    parts_ = workers_ + 1;
    chunk_ = ((bytes + (size_t)parts_ - 1) / (size_t)parts_ + 4095) & ~size_t(4095);
    next_ = done_ = 0;
    wake_.notify_all();
    work(lk);
    finished_.wait(lk, [&] { return done_ == parts_; });
    parts_ = 0;
  }

 private:
  static std::atomic<bool>& forked() {
    static std::atomic<bool> f{false};
    return f;
  }
  CopyPool() {
    (void)pthread_atfork(nullptr, nullptr, [] { forked().store(true, std::memory_order_relaxed); });
    const char* e = std::getenv("RIP_COPY_THREADS");  // worker threads beside the caller; 0 = plain memcpy
    const int hw = (int)std::thread::hardware_concurrency();
    workers_ = e ? std::max(0, std::min(16, std::atoi(e))) : std::max(0, std::min(3, hw - 1));
    for (int i = 0; i < workers_; i++)
      std::thread([this] {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
          wake_.wait(lk, [&] { return next_ < parts_; });
          work(lk);
        }
      }).detach();
  }
  // claims parts of the current copy until none is left; called and left with the lock held
  void work(std::unique_lock<std::mutex>& lk) {
    while (next_ < parts_) {
      const size_t off = (size_t)next_++ * chunk_;
      uint8_t* d = dst_;
      const uint8_t* s = src_;
      const size_t n = off < bytes_ ? std::min(chunk_, bytes_ - off) : 0;
      lk.unlock();
      if (n) std::memcpy(d + off, s + off, n);
      lk.lock();
      if (++done_ == parts_) finished_.notify_all();
    }
  }
  std::mutex busy_, mu_;
  std::condition_variable wake_, finished_;
  uint8_t* dst_ = nullptr;
  const uint8_t* src_ = nullptr;
  size_t bytes_ = 0, chunk_ = 0;
  int parts_ = 0, next_ = 0, done_ = 0, workers_ = 0;
};

// Device-wide limit on the host frames in flight (rip_submit).  Measured on MI355X / ROCm 7.2 (tools/probes/ring_depth_probe.py,
// rig_ring_probe.py, EXPERIMENTS.md): with three frames' uploads, kernels and downloads enqueued on their streams a 15 MB
// download takes 0.295 ms; from the fourth frame on -- one handle with a deeper ring, or several handles on one device -- some
// downloads take 1.19 ms or several ms (the runtime's handling of cross-stream dependencies of SDMA copies under direct
// dispatch: the effect is gone with AMD_DIRECT_DISPATCH=0), and the whole pipeline runs at half its rate.  So rip_submit
// waits for the oldest frame in flight on the device to finish before it enqueues a fourth one -- work that has to finish
// before the new frame's download can start anyway.  RIP_RING_INFLIGHT changes the limit (0 = none).
struct InflightGate {
  // One mutex and one queue per device: a submit that waits at the limit on device 0 holds device 0's lock only;
  // submits and collects of handles on the other devices of a multi-GPU rig go on.
  std::mutex mu[64];
  std::deque<hipEvent_t> q[64];  // per device: ev_done of the frames enqueued and not yet known to be complete, oldest first
  int cap() {
    static const int c = [] {
      const char* e = std::getenv("RIP_RING_INFLIGHT");
      return e ? std::max(0, std::atoi(e)) : 3;
    }();
    return c;
  }
  void admit(int device) {
    const int c = cap();
    if (c <= 0) return;
    // The wait happens under the DEVICE's lock on purpose: an event in the queue belongs to some handle's slot, and forget() --
    // called before a slot's events are destroyed or recorded again -- must not get past it while it is waited on.  The wait
    // is for a frame that is already enqueued in full (at most one frame time), and whoever else wants this device's lock
    // meanwhile is either about to wait for the same frame (another submit at the limit) or finishes a collect a moment later.
    std::lock_guard<std::mutex> lk(mu[device & 63]);
    auto& d = q[device & 63];
    while ((int)d.size() >= c) {
      hipEvent_t e = d.front();
      d.pop_front();
      (void)hipEventSynchronize(e);
    }
  }
  void enqueued(int device, hipEvent_t e) {
    if (cap() <= 0) return;
    std::lock_guard<std::mutex> lk(mu[device & 63]);
    q[device & 63].push_back(e);
  }
  // the frame is complete, or its event is about to be destroyed / recorded again.  device: where it was enqueued (< 0: never)
  void forget(int device, hipEvent_t e) {
    if (!e || device < 0) return;
    std::lock_guard<std::mutex> lk(mu[device & 63]);
    auto& d = q[device & 63];
    for (auto it = d.begin(); it != d.end();) it = (*it == e) ? d.erase(it) : it + 1;
  }
};
InflightGate& inflight_gate() {
  static InflightGate g;
  return g;
}

}  // namespace

void RingSlot::release() {
    if (h_out) (void)hipHostFree(h_out);
    h_out = nullptr;
    h_out_cap = 0;
    if (h_in) (void)hipHostFree(h_in);
    h_in = nullptr;
    h_in_cap = 0;
    for (int i = 0; i < 2; i++) {
      if (h_tap[i]) (void)hipHostFree(h_tap[i]);
      h_tap[i] = nullptr;
      h_tap_cap[i] = 0;
    }
    inflight_gate().forget(gate_device, ev_done);
    gate_device = -1;
    for (hipEvent_t* e : {&ev_up, &ev_kernels, &ev_done, &ev_start, &ev_dl_start}) {
      if (*e) (void)hipEventDestroy(*e);
      *e = nullptr;
    }
    for (DevBuf* b : {&d_in, &d_out, &d_tap_deb, &d_tap_col}) b->release();
  }

namespace {

// true for hipHostMalloc'd / hipHostRegister'ed memory (the runtime can DMA from it without a staging copy)
bool host_pointer_is_pinned(const void* ptr) {
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
    (void)hipGetLastError();  // older runtimes report an ordinary malloc'd pointer as an error
    return false;
  }
  return at.type == hipMemoryTypeHost;
}

// What a host frame call needs to know about one frame: the caller's row pitch (resolved), the payload bytes of an input row, the
// staging geometry on the device (dword-aligned rows), the sizes of the delivered image and of a tap, and which taps are kept
struct HostFrameLayout {
  size_t step, in_row, in_pitch, in_bytes, out_bytes, mid_bytes;
  bool keep_deb, keep_col;  // rip_set_taps; bgr16 results have no taps
  HostFrameLayout(const rip_pipeline* p, const Plan& pl, int rows, int cols, int channels, size_t caller_step)
      : step(caller_step), in_row(row_bytes(pl, cols, channels)), in_pitch((in_row + 3) & ~(size_t)3), in_bytes(in_pitch * rows),
        out_bytes(delivered_bytes(pl)), mid_bytes((size_t)pl.mid_rows * pl.mid_cols * pl.channels),
        keep_deb((p->tap_mask & RIP_TAP_DEBAYERED) && pl.out_elem_bytes == 1), keep_col((p->tap_mask & RIP_TAP_COLOR) && pl.out_elem_bytes == 1) {
    if (step == 0) step = in_row;
  }
  // packed rows are copied whole, whatever the pitch says
  void check_step(const Plan& pl) const {
    if (pl.packed_layout && step < in_row) throw InvalidArgument("input row pitch smaller than a row");
  }
  ConstFrameView staged(const void* d_in, int rows, int cols) const { return {static_cast<const uint8_t*>(d_in), in_pitch, in_bytes, rows, cols}; }
  // the delivered image at d_out, tightly packed: under a format with the checks of rip_apply_device, native as it lies
  static FrameView delivered(const Plan& pl, void* d_out) {
    return pl.out_fmt != rip::OUT_NATIVE ? resolve_output_layout(pl, d_out, 0, 0) : tight_output_view(pl, d_out);
  }
};

// what rip_get_image / rip_get_image_view hand out for image `which`: buf on the device, host where a pinned copy exists
void remember_last(rip_pipeline* p, int which, DevBuf* buf, const void* host, int rows, int cols, int channels, bool on) {
  p->last_valid[which] = on;
  p->last_buf[which] = buf;
  p->last_host[which] = host;
  p->last_rows[which] = rows;
  p->last_cols[which] = cols;
  p->last_cn[which] = channels;
}

// RIP_IMAGE_RECT_MASK holds something: a mode other than "off", and the last frame call's frame was undistorted -- by an undistortion
// that still exists (the mask is built from the current maps when a getter asks)
bool rect_mask_exists(const rip_pipeline* p) {
  return p->m.rect_mask != "off" && p->mask_frame.remap && p->m.und_available && p->m.dist_model != "none" && p->m.dist_w > 0 && p->m.dist_h > 0;
}

rip_status submit_impl(rip_pipeline* p, const uint8_t* image, int rows, int cols, int channels, size_t step, const char* encoding,
                       uint8_t* ext_out, size_t ext_out_capacity, uint8_t* ext_deb, uint8_t* ext_col, size_t ext_tap_capacity,
                       uint64_t* ticket) {
  return guarded(p, [&] {
    need_device(p);
    if (!image || !encoding || !ticket) throw InvalidArgument("null buffer, encoding or ticket");
    const Plan pl = delivered_plan(p, rows, cols, channels, encoding);  // a null encoding was refused above
    if (rip::output_format_jpeg(pl.out_fmt))
      throw InvalidArgument("rip_submit: the output format [jpeg] delivers streams of a length the ring does not carry; use rip_apply, rip_apply_heads or the device calls");
    const HostFrameLayout L(p, pl, rows, cols, channels, step);
    {  // destinations given by the caller (rip_submit_to): checked before anything is enqueued or any slot is touched
      if (ext_out && ext_out_capacity < L.out_bytes) throw CapacityError("rip_submit_to: result buffer too small: need " + std::to_string(L.out_bytes) + " bytes");
      if ((ext_deb || ext_col) && ext_tap_capacity < L.mid_bytes) throw CapacityError("rip_submit_to: tap buffer too small: need " + std::to_string(L.mid_bytes) + " bytes");
      if (ext_deb && !L.keep_deb) throw InvalidArgument("rip_submit_to: the debayered tap is not kept (rip_set_taps)");
      if (ext_col && !L.keep_col) throw InvalidArgument("rip_submit_to: the colour tap is not kept (rip_set_taps)");
      for (const void* ptr : {(const void*)ext_out, (const void*)ext_deb, (const void*)ext_col})
        if (ptr && !host_pointer_is_pinned(ptr))
          throw InvalidArgument("rip_submit_to: destination buffers must be page-locked (rip_host_alloc, hipHostMalloc, hipHostRegister)");
    }
    DeviceGuard device_guard(p->device);
    if (!p->ul_stream) HIP_CHECK(hipStreamCreateWithFlags(&p->ul_stream, hipStreamNonBlocking));
    if (!p->dl_stream) HIP_CHECK(hipStreamCreateWithFlags(&p->dl_stream, hipStreamNonBlocking));
    while ((int)p->ring.size() < p->ring_depth) {
      std::unique_ptr<RingSlot> sl(new RingSlot());
      static const bool debug_ring = std::getenv("RIP_DEBUG_RING") != nullptr;  // development aid: per-frame upload / kernel / download times on stderr
      for (hipEvent_t* e : {&sl->ev_up, &sl->ev_kernels, &sl->ev_done}) HIP_CHECK(hipEventCreateWithFlags(e, debug_ring ? hipEventDefault : hipEventDisableTiming));
      if (debug_ring) HIP_CHECK(hipEventCreateWithFlags(&sl->ev_start, hipEventDefault));
      if (debug_ring) HIP_CHECK(hipEventCreateWithFlags(&sl->ev_dl_start, hipEventDefault));
      p->ring.push_back(std::move(sl));
    }
    // a free slot; failing that the slot of the frame collected last (its view and taps end here); failing that: full
    RingSlot* pick = nullptr;
    uint64_t oldest = ~0ull;
    for (auto& c : p->ring)
      if (!c->busy && !c->held) pick = c.get();
    if (!pick)
      for (auto& c : p->ring) {
        if (c->held) pick = c.get();
        if (c->busy) oldest = std::min(oldest, c->ticket);
      }
    if (!pick)
      throw CapacityError("rip_submit: " + std::to_string(p->ring_depth) + " frames are in flight; collect ticket " +
                          std::to_string(oldest) + " first (or raise rip_set_ring_depth)");
    RingSlot& sl = *pick;
    if (sl.held) {
      sl.held = false;
      for (int i = 0; i < 3; i++)
        if (p->last_buf[i] == &sl.d_tap_deb || p->last_buf[i] == &sl.d_tap_col || p->last_buf[i] == &sl.d_out) p->last_valid[i] = false;
    }
    L.check_step(pl);
    sl.d_in.reserve(L.in_bytes);
    sl.d_out.reserve(L.out_bytes);
    if (!ext_out) sl.reserve_host(L.out_bytes);
    sl.has_deb = L.keep_deb;
    sl.has_col = L.keep_col;
    sl.dl_deb = sl.has_deb && ((p->tap_download_mask & RIP_TAP_DEBAYERED) || ext_deb);
    sl.dl_col = sl.has_col && ((p->tap_download_mask & RIP_TAP_COLOR) || ext_col);
    if (sl.has_deb) sl.d_tap_deb.reserve(L.mid_bytes);
    if (sl.has_col) sl.d_tap_col.reserve(L.mid_bytes);
    if (sl.dl_deb && !ext_deb) RingSlot::reserve_pinned(sl.h_tap[0], sl.h_tap_cap[0], L.mid_bytes);
    if (sl.dl_col && !ext_col) RingSlot::reserve_pinned(sl.h_tap[1], sl.h_tap_cap[1], L.mid_bytes);
    sl.dst_out = ext_out ? (void*)ext_out : sl.h_out;
    sl.dst_tap[0] = ext_deb ? (void*)ext_deb : sl.h_tap[0];
    sl.dst_tap[1] = ext_col ? (void*)ext_col : sl.h_tap[1];
    // upload (its own stream: it overlaps the kernels of the frame before) -> kernels on the handle's stream, in submission
    // order -> download into the slot's pinned buffer (its own stream: it overlaps the kernels of the frame after)
    // A frame in pinned memory (rip_host_alloc, hipHostMalloc, hipHostRegister) is DMA'd from where it lies and must stay
    // untouched until its ticket is collected.  Anything else is copied into the slot's pinned staging buffer first, so the
    // caller's buffer is free again when this call returns whatever the runtime does with an asynchronous 2-D copy from
    // pageable memory (above its staging threshold it pins the pages in place and copies after the call has returned).
    inflight_gate().forget(sl.gate_device, sl.ev_done);  // the slot's previous frame (collected, or it would not have been picked)
    inflight_gate().admit(p->device);
    if (sl.ev_start) HIP_CHECK(hipEventRecord(sl.ev_start, p->ul_stream));
    if (host_pointer_is_pinned(image)) {
      HIP_CHECK(hipMemcpy2DAsync(sl.d_in.ptr, L.in_pitch, image, L.step, L.in_row, (size_t)rows, hipMemcpyHostToDevice, p->ul_stream));
    } else {
      sl.reserve_host_in(L.in_bytes);
      uint8_t* stage = static_cast<uint8_t*>(sl.h_in);
      if (L.step == L.in_pitch) {
        CopyPool::get().copy(stage, image, L.in_pitch * (size_t)(rows - 1) + L.in_row);
      } else {
        for (int r = 0; r < rows; r++) std::memcpy(stage + (size_t)r * L.in_pitch, image + (size_t)r * L.step, L.in_row);
      }
      HIP_CHECK(hipMemcpyAsync(sl.d_in.ptr, stage, L.in_bytes, hipMemcpyHostToDevice, p->ul_stream));
    }
    HIP_CHECK(hipEventRecord(sl.ev_up, p->ul_stream));
    HIP_CHECK(hipStreamWaitEvent(p->stream, sl.ev_up, 0));
    begin_jpeg_call(p, pl, 1);  // no jpeg head gets here: the head's stream lengths of an earlier call end
    run_batch_formatted(p, pl, L.staged(sl.d_in.ptr, rows, cols), HostFrameLayout::delivered(pl, sl.d_out.ptr),
                        {sl.has_deb ? sl.d_tap_deb.as<uint8_t>() : nullptr, sl.has_col ? sl.d_tap_col.as<uint8_t>() : nullptr}, 1);
    HIP_CHECK(hipEventRecord(sl.ev_kernels, p->stream));
    HIP_CHECK(hipStreamWaitEvent(p->dl_stream, sl.ev_kernels, 0));
    if (sl.ev_dl_start) HIP_CHECK(hipEventRecord(sl.ev_dl_start, p->dl_stream));
    HIP_CHECK(hipMemcpyAsync(sl.dst_out, sl.d_out.ptr, L.out_bytes, hipMemcpyDeviceToHost, p->dl_stream));
    // the taps rip_set_tap_download names travel with the result: a per-frame caller that publishes them
    // (raw_image_pipeline_ros.cpp:245-287: up to three images per callback) gets them from pinned host memory instead of
    // one synchronous device read each (rip_get_image / rip_get_image_view after rip_collect).  Off by default: a caller that
    // only wants the final image must not pay 30 MB more PCIe traffic per 2448 x 2048 frame.
    if (sl.dl_deb) HIP_CHECK(hipMemcpyAsync(sl.dst_tap[0], sl.d_tap_deb.ptr, L.mid_bytes, hipMemcpyDeviceToHost, p->dl_stream));
    if (sl.dl_col) HIP_CHECK(hipMemcpyAsync(sl.dst_tap[1], sl.d_tap_col.ptr, L.mid_bytes, hipMemcpyDeviceToHost, p->dl_stream));
    HIP_CHECK(hipEventRecord(sl.ev_done, p->dl_stream));
    inflight_gate().enqueued(p->device, sl.ev_done);
    sl.gate_device = p->device;
    sl.pl = pl;
    sl.ticket = p->next_ticket++;
    sl.busy = true;
    *ticket = sl.ticket;
  });
}

}  // namespace
}  // namespace rip::api

using namespace rip::api;

#pragma GCC visibility push(default)
extern "C" {

rip_status rip_apply(rip_pipeline* p, const uint8_t* image, int rows, int cols, int channels, size_t step, const char* encoding,
                     uint8_t* out, size_t out_capacity, int* out_rows, int* out_cols, int* out_channels,
                     char encoding_out[32]) {
  return guarded(p, [&] {
    need_device(p);
    if (!image || !out || !encoding) throw InvalidArgument("null buffer or encoding");
    const Plan pl = delivered_plan(p, rows, cols, channels, encoding);  // a null encoding was refused above
    DeviceGuard device_guard(p->device);
    const HostFrameLayout L(p, pl, rows, cols, channels, step);
    L.check_step(pl);
    if (out_capacity < L.out_bytes) throw CapacityError("output buffer too small: need " + std::to_string(L.out_bytes) + " bytes");
    p->d_in.reserve(L.in_bytes);
    p->d_out.reserve(L.out_bytes);
    if (L.keep_deb) p->d_tap_deb.reserve(L.mid_bytes);
    if (L.keep_col) p->d_tap_col.reserve(L.mid_bytes);
    const Taps taps = {L.keep_deb ? p->d_tap_deb.as<uint8_t>() : nullptr, L.keep_col ? p->d_tap_col.as<uint8_t>() : nullptr};
    const ConstFrameView src = L.staged(p->d_in.ptr, rows, cols);
    HIP_CHECK(hipMemcpy2DAsync(p->d_in.ptr, L.in_pitch, image, L.step, L.in_row, (size_t)rows, hipMemcpyHostToDevice, p->stream));
    begin_jpeg_call(p, pl, 1);
    run_batch_formatted(p, pl, src, HostFrameLayout::delivered(pl, p->d_out.ptr), taps, 1);
    if (rip::output_format_jpeg(pl.out_fmt)) download_jpeg_frame(p, pl, p->d_out.ptr, out);  // the length first, then the used bytes
    else HIP_CHECK(hipMemcpyAsync(out, p->d_out.ptr, L.out_bytes, hipMemcpyDeviceToHost, p->stream));
    HIP_CHECK(hipStreamSynchronize(p->stream));
    const bool eb1 = pl.out_elem_bytes == 1;
    if (p->m.debug && eb1) {
      if (pl.out_fmt == rip::OUT_NATIVE && !pl.rsz_active && !pl.clahe) {
        write_debug_dumps(p, pl, src, out);
      } else {  // the dumps show the pipeline's image, not the delivered buffer: fetch it from the staging buffer
        const size_t row = (size_t)pl.out_cols * pl.channels;
        std::vector<uint8_t> native(row * pl.out_rows);
        HIP_CHECK(hipMemcpy2DAsync(native.data(), row, p->d_fmt.ptr, fmt_pitch(pl), row, (size_t)pl.out_rows,
                                   hipMemcpyDeviceToHost, p->stream));
        HIP_CHECK(hipStreamSynchronize(p->stream));
        write_debug_dumps(p, pl, src, native.data());
      }
    }
    for (int i = 0; i < 3; i++) p->last_valid[i] = false;
    remember_last(p, RIP_IMAGE_DEBAYERED, &p->d_tap_deb, nullptr, pl.mid_rows, pl.mid_cols, pl.channels, L.keep_deb);
    remember_last(p, RIP_IMAGE_COLOR, &p->d_tap_col, nullptr, pl.mid_rows, pl.mid_cols, pl.channels, L.keep_col);
    // under a format, a resize or CLAHE the delivered buffer is the result (as for bgr16): no PROCESSED image
    remember_last(p, RIP_IMAGE_PROCESSED, &p->d_out, nullptr, pl.out_rows, pl.out_cols, pl.channels, (p->tap_mask & RIP_TAP_PROCESSED) != 0 && eb1 && !pl.fmt_active && !pl.rsz_active && !pl.clahe);
    remember_mask_frame(p, pl);
    if (out_rows) *out_rows = pl.dl_rows;
    if (out_cols) *out_cols = pl.dl_cols;
    if (out_channels) *out_channels = pl.dl_channels;
    if (encoding_out) copy_string(pl.encoding_out, encoding_out, 32);
  });
}

// rip_apply with several delivered images: one upload, one run of the chain, one download per requested head.  No debug dumps are
// written from here (rip_set_debug is for the single-output calls: the dumps re-run the chain per module).
rip_status rip_apply_heads(rip_pipeline* p, const uint8_t* image, int rows, int cols, int channels, size_t step, const char* encoding,
                           uint8_t* const* outs, const size_t* out_capacities, int n_heads, int* out_rows, int* out_cols, int* out_channels) {
  return guarded(p, [&] {
    need_device(p);
    if (!image || !outs || !out_capacities || !encoding) throw InvalidArgument("null buffer, heads or encoding");
    if (n_heads != p->m.n_heads)
      throw InvalidArgument("rip_apply_heads: " + std::to_string(n_heads) + " head buffers for a handle with " + std::to_string(p->m.n_heads) + " output heads");
    bool requested[RIP_MAX_OUTPUT_HEADS] = {};
    bool any = false;
    for (int k = 0; k < n_heads; k++) any |= requested[k] = outs[k] != nullptr;
    if (!any) throw InvalidArgument("rip_apply_heads: no head is requested (every output buffer is null)");
    const Plan pl = make_plan(p->m, rows, cols, channels, encoding);
    const HostFrameLayout L(p, pl, rows, cols, channels, step);
    Plan plans[RIP_MAX_OUTPUT_HEADS];
    FrameView dsts[RIP_MAX_OUTPUT_HEADS];
    // the delivered image of a head, tightly packed behind a fixed 16-byte aligned address: the checks need no allocation, the
    // buffers are reserved once every head has passed
    plan_heads(p->m, pl, n_heads, requested, false, plans, dsts, [&](int k, const Plan& hp) {
      if (out_capacities[k] < delivered_bytes(hp)) throw CapacityError("output buffer too small: need " + std::to_string(delivered_bytes(hp)) + " bytes");
      return HostFrameLayout::delivered(hp, reinterpret_cast<void*>(uintptr_t(4096)));
    });
    L.check_step(pl);
    DeviceGuard device_guard(p->device);
    p->d_in.reserve(L.in_bytes);
    for (int k = 0; k < n_heads; k++) {
      if (!requested[k]) continue;
      p->d_head_out[k].reserve(delivered_bytes(plans[k]));
      dsts[k].ptr = p->d_head_out[k].as<uint8_t>();
    }
    if (L.keep_deb) p->d_tap_deb.reserve(L.mid_bytes);
    if (L.keep_col) p->d_tap_col.reserve(L.mid_bytes);
    const Taps taps = {L.keep_deb ? p->d_tap_deb.as<uint8_t>() : nullptr, L.keep_col ? p->d_tap_col.as<uint8_t>() : nullptr};
    const ConstFrameView src = L.staged(p->d_in.ptr, rows, cols);
    HIP_CHECK(hipMemcpy2DAsync(p->d_in.ptr, L.in_pitch, image, L.step, L.in_row, (size_t)rows, hipMemcpyHostToDevice, p->stream));
    for (int k = 0; k < n_heads; k++)
      if (requested[k]) begin_jpeg_call(p, plans[k], 1);
    run_batch_heads(p, pl, plans, dsts, n_heads, src, taps, 1);
    for (int k = 0; k < n_heads; k++) {
      if (!requested[k]) continue;
      if (rip::output_format_jpeg(plans[k].out_fmt)) download_jpeg_frame(p, plans[k], p->d_head_out[k].ptr, outs[k]);
      else HIP_CHECK(hipMemcpyAsync(outs[k], p->d_head_out[k].ptr, delivered_bytes(plans[k]), hipMemcpyDeviceToHost, p->stream));
    }
    HIP_CHECK(hipStreamSynchronize(p->stream));
    for (int i = 0; i < 3; i++) p->last_valid[i] = false;
    remember_last(p, RIP_IMAGE_DEBAYERED, &p->d_tap_deb, nullptr, pl.mid_rows, pl.mid_cols, pl.channels, L.keep_deb);
    remember_last(p, RIP_IMAGE_COLOR, &p->d_tap_col, nullptr, pl.mid_rows, pl.mid_cols, pl.channels, L.keep_col);
    // the delivered buffers are the results: no PROCESSED image
    remember_last(p, RIP_IMAGE_PROCESSED, &p->d_out, nullptr, pl.out_rows, pl.out_cols, pl.channels, false);
    remember_mask_frame(p, pl);
    for (int k = 0; k < n_heads; k++) {
      if (out_rows) out_rows[k] = requested[k] ? plans[k].dl_rows : 0;
      if (out_cols) out_cols[k] = requested[k] ? plans[k].dl_cols : 0;
      if (out_channels) out_channels[k] = requested[k] ? plans[k].dl_channels : 0;
    }
  });
}

rip_status rip_submit(rip_pipeline* p, const uint8_t* image, int rows, int cols, int channels, size_t step, const char* encoding,
                      uint64_t* ticket) {
  return submit_impl(p, image, rows, cols, channels, step, encoding, nullptr, 0, nullptr, nullptr, 0, ticket);
}
rip_status rip_submit_to(rip_pipeline* p, const uint8_t* image, int rows, int cols, int channels, size_t step, const char* encoding,
                         uint8_t* out, size_t out_capacity, uint8_t* tap_debayered, uint8_t* tap_color, size_t tap_capacity, uint64_t* ticket) {
  return submit_impl(p, image, rows, cols, channels, step, encoding, out, out_capacity, tap_debayered, tap_color, tap_capacity, ticket);
}

rip_status rip_collect(rip_pipeline* p, uint64_t ticket, uint8_t* out, size_t out_capacity, const uint8_t** out_view, int* out_rows,
                       int* out_cols, int* out_channels, char encoding_out[32]) {
  return guarded(p, [&] {
    need_device(p);
    RingSlot* sl = nullptr;
    for (auto& s : p->ring)
      if (s->busy && s->ticket == ticket) sl = s.get();
    if (!sl) throw InvalidArgument("rip_collect: ticket " + std::to_string(ticket) + " is not in flight");
    const Plan& pl = sl->pl;
    const size_t out_bytes = delivered_bytes(pl);
    if (out && out_capacity < out_bytes) throw CapacityError("output buffer too small: need " + std::to_string(out_bytes) + " bytes");
    DeviceGuard device_guard(p->device);
    HIP_CHECK(hipEventSynchronize(sl->ev_done));
    inflight_gate().forget(sl->gate_device, sl->ev_done);
    if (sl->ev_start) {
      float up = 0, kern = 0, down = 0, all = 0, copy = 0;
      (void)hipEventElapsedTime(&copy, sl->ev_dl_start, sl->ev_done);
      (void)hipEventElapsedTime(&up, sl->ev_start, sl->ev_up);
      (void)hipEventElapsedTime(&kern, sl->ev_up, sl->ev_kernels);
      (void)hipEventElapsedTime(&down, sl->ev_kernels, sl->ev_done);
      (void)hipEventElapsedTime(&all, sl->ev_start, sl->ev_done);
      int idx = 0;
      for (size_t i = 0; i < p->ring.size(); i++)
        if (p->ring[i].get() == sl) idx = (int)i;
      std::fprintf(stderr, "rip ring: ticket %llu slot %d upload %.3f ms, kernels (incl. waiting for the frame before) %.3f, download (incl. waiting) %.3f of which the copies %.3f, total %.3f\n",
                   (unsigned long long)ticket, idx, up, kern, down, copy, all);
    }
    if (out && out != sl->dst_out) CopyPool::get().copy(out, sl->dst_out, out_bytes);
    if (out_view) *out_view = static_cast<const uint8_t*>(sl->dst_out);
    for (auto& c : p->ring) c->held = false;  // the frame collected before this one lets go of its slot
    sl->busy = false;
    sl->held = true;
    const bool eb1 = pl.out_elem_bytes == 1;
    // The getters may read a host copy only where it is the HANDLE's pinned buffer.  Destinations the caller named
    // (rip_submit_to) are the caller's again from this point on -- rip.h only asks for them until the ticket is collected:
    // they may be freed or edited, so the getters go back to the device image in the slot this frame keeps held.
    remember_last(p, RIP_IMAGE_DEBAYERED, &sl->d_tap_deb, sl->dl_deb && sl->dst_tap[0] == sl->h_tap[0] ? sl->dst_tap[0] : nullptr, pl.mid_rows, pl.mid_cols, pl.channels, sl->has_deb);
    remember_last(p, RIP_IMAGE_COLOR, &sl->d_tap_col, sl->dl_col && sl->dst_tap[1] == sl->h_tap[1] ? sl->dst_tap[1] : nullptr, pl.mid_rows, pl.mid_cols, pl.channels, sl->has_col);
    remember_last(p, RIP_IMAGE_PROCESSED, &sl->d_out, sl->dst_out == sl->h_out ? sl->dst_out : nullptr, pl.out_rows, pl.out_cols, pl.channels, (p->tap_mask & RIP_TAP_PROCESSED) != 0 && eb1 && !pl.fmt_active && !pl.rsz_active && !pl.clahe);
    remember_mask_frame(p, pl);
    if (out_rows) *out_rows = pl.dl_rows;
    if (out_cols) *out_cols = pl.dl_cols;
    if (out_channels) *out_channels = pl.dl_channels;
    if (encoding_out) copy_string(pl.encoding_out, encoding_out, 32);
  });
}

rip_status rip_set_ring_depth(rip_pipeline* p, int depth) {
  return guarded(p, [&] {
    need(p);
    if (depth < 1 || depth > 16) throw InvalidArgument("ring depth must be in 1..16");
    for (auto& s : p->ring)
      if (s->busy) throw InvalidArgument("rip_set_ring_depth: frames are in flight");
    if (depth == p->ring_depth) return;
    if (!p->ring.empty()) {
      DeviceGuard device_guard(p->device);
      for (int i = 0; i < 3; i++)  // the getters must not look into a slot that is about to go
        for (auto& s : p->ring)
          if (p->last_buf[i] == &s->d_tap_deb || p->last_buf[i] == &s->d_tap_col || p->last_buf[i] == &s->d_out) p->last_valid[i] = false;
      if (p->dl_stream) HIP_CHECK(hipStreamSynchronize(p->dl_stream));
      for (auto& s : p->ring) s->release();
      p->ring.clear();
    }
    p->ring_depth = depth;
  });
}

void* rip_host_alloc(size_t bytes) {
  void* ptr = nullptr;
  if (bytes == 0 || hipHostMalloc(&ptr, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return ptr;
}
void rip_host_free(void* ptr) {
  if (ptr) (void)hipHostFree(ptr);
}
void rip_copy_host(void* dst, const void* src, size_t bytes) {
  if (dst && src && bytes) CopyPool::get().copy(dst, src, bytes);
}

rip_status rip_get_image(rip_pipeline* p, int which, uint8_t* out, size_t out_capacity, int* rows, int* cols, int* channels) {
  return guarded(p, [&] {
    need(p);
    if (which == RIP_IMAGE_RECT_MASK && rect_mask_exists(p)) {
      // built here, on demand, from the maps and the size of the image that entered the last frame's remap (PARITY.md "Rect mask")
      const int mrows = p->m.dist_h, mcols = p->m.dist_w;
      const size_t bytes = (size_t)mrows * (size_t)mcols;
      if (rows) *rows = mrows;
      if (cols) *cols = mcols;
      if (channels) *channels = 1;
      if (!out) return;  // size query
      if (out_capacity < bytes) throw CapacityError("image buffer too small");
      need_device(p);
      DeviceGuard device_guard(p->device);
      const ConstFrameView m = ensure_mask_base(p, true, p->mask_frame.src_rows, p->mask_frame.src_cols, mrows, mcols, p->m.rect_mask == "valid");
      HIP_CHECK(hipMemcpy2DAsync(out, (size_t)mcols, m.ptr, m.step, (size_t)mcols, (size_t)mrows, hipMemcpyDeviceToHost, p->stream));
      HIP_CHECK(hipStreamSynchronize(p->stream));
      return;
    }
    if (which == RIP_IMAGE_RECT_MASK || which < 0 || which > 3 || !p->last_valid[which]) {
      // the reference never writes rect_mask_, and neither does this library under the mode "off"; taps that were not kept are empty too
      if (which < 0 || which > 3) throw InvalidArgument("unknown image id");
      if (rows) *rows = 0;
      if (cols) *cols = 0;
      if (channels) *channels = 0;
      return;
    }
    size_t bytes = (size_t)p->last_rows[which] * p->last_cols[which] * p->last_cn[which];
    if (rows) *rows = p->last_rows[which];
    if (cols) *cols = p->last_cols[which];
    if (channels) *channels = p->last_cn[which];
    if (!out) return;  // size query
    if (out_capacity < bytes) throw CapacityError("image buffer too small");
    need_device(p);
    if (p->last_host[which]) {  // a frame that came through rip_collect: the image is in pinned host memory already
      CopyPool::get().copy(out, p->last_host[which], bytes);
      return;
    }
    DeviceGuard device_guard(p->device);
    HIP_CHECK(hipMemcpyAsync(out, p->last_buf[which]->ptr, bytes, hipMemcpyDeviceToHost, p->stream));
    HIP_CHECK(hipStreamSynchronize(p->stream));
  });
}

rip_status rip_get_image_view(rip_pipeline* p, int which, const uint8_t** view, int* rows, int* cols, int* channels) {
  return guarded(p, [&] {
    need(p);
    if (!view) throw InvalidArgument("null view");
    if (which < 0 || which > 3) throw InvalidArgument("unknown image id");
    *view = nullptr;
    if (which == RIP_IMAGE_RECT_MASK) {  // the mask lives on the device: its geometry with a null view, or empty
      const bool mask = rect_mask_exists(p);
      if (rows) *rows = mask ? p->m.dist_h : 0;
      if (cols) *cols = mask ? p->m.dist_w : 0;
      if (channels) *channels = mask ? 1 : 0;
      return;
    }
    const bool have = p->last_valid[which];
    if (rows) *rows = have ? p->last_rows[which] : 0;
    if (cols) *cols = have ? p->last_cols[which] : 0;
    if (channels) *channels = have ? p->last_cn[which] : 0;
    if (have) *view = static_cast<const uint8_t*>(p->last_host[which]);
  });
}

}  // extern "C"
#pragma GCC visibility pop
