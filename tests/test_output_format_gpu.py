"""The output stage on the GPU (include/rip.h rip_set_output_format): what the frame calls deliver equals
``output_reference.convert(E, format, normalisation)`` bit for bit -- floats compared as bit patterns -- where E is the image the
suite already trusts for that input (helpers.oracle_run, expected_mht, expected_raw16), and not one byte outside the delivered
elements is written.

Widths come from the converter's constants (rip_output.hpp: 4 pixels per lane, 256 lanes = 1024 pixels per workgroup): 3, 5, 7
end in a partial lane, 4 and 8 in a full one; 1021, 1025, 1027 and 2051 put the partial lane before, right behind and behind a
workgroup boundary, 1024 fills a workgroup exactly.  Tight planes of an odd width change their alignment from row to row and from
plane to plane, which is what decides between the wide and the single-element stores.  Heights are 3 to 5 rows."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import output_reference as R
import output_variant_cases as OV
import packed_reference as PKR
import raw16_cases as G
import variant_cases as V
from helpers import assert_launched, cfg, configure, expected_mht, oracle_params, oracle_run
from raw16_reference import demosaic16, expected_raw16
from raw_image_pipeline_amd import RawImagePipeline, synth
from raw_image_pipeline_amd import pipeline as P
from test_cpp_facade import BRANCHES, run_env
from test_output_format import build_output_format_test

pytestmark = pytest.mark.gpu

WIDTHS = (3, 4, 5, 7, 8, 1021, 1024, 1025, 1027, 2051)
NORM = OV.NORM
SENTINEL = 0xA5
PITCHES = ("tight", "pitch16", "pitch_elem")


def torch_dtype(fmt):
    import torch
    return {"rgb8": torch.uint8, "mono8": torch.uint8, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[
        fmt if fmt in ("rgb8", "mono8") else fmt.rsplit("_", 1)[1]]


@functools.lru_cache(maxsize=None)
def bgr_frames(w, h, n, seed=0):
    """n different bgr8 frames: uniform noise (every byte value, every neighbourhood).  Shared; read-only."""
    f = np.random.default_rng(1000 + seed + 7 * w + h).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def identity_expectation(oracle_id, w, h, n, seed=0):
    """E of bgr_frames under a configuration with every stage off, from the oracle.  Shared; read-only."""
    import oracle as O
    e = np.stack([oracle_run(O, cfg(), np.ascontiguousarray(f), "bgr8")[0] for f in bgr_frames(w, h, n, seed)])
    e.setflags(write=False)
    return e


def plain_pipe(fmt, norm=NORM):
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, cfg())
    pipe.set_output_format(fmt)
    pipe.set_output_normalization(*norm)
    return pipe


class Destination:
    """A delivered batch as a strided view of one flat buffer of SENTINEL bytes, on the device (``view``) and as the host's
    expectation of every byte of that buffer (``expected_bytes``): the converted frames where the view lies, sentinels elsewhere."""

    def __init__(self, fmt, n, rows, cols, pitch="tight", gap=False, base_off=False, on_device=True):
        elem = R.ELEM_BYTES[fmt]
        planar = R.is_planar(fmt)
        row = cols * (1 if planar or fmt == "mono8" else 3)           # elements of one row
        if pitch == "tight":
            step = row
        elif pitch == "pitch16":                                          # a multiple of 16 bytes
            step = ((row * elem + 15) // 16 * 16 + 16) // elem
        else:                                                             # element-aligned, no multiple of 16 bytes
            step = row + 1
            if step * elem % 16 == 0:
                step += 1
        frame = step * rows * (3 if planar else 1) + (5 if gap else 0)   # the gap: an odd number of elements
        offset = 1 if base_off else 0
        total = offset + frame * n + 3
        self.fmt, self.elem, self.step_bytes, self.frame_bytes = fmt, elem, step * elem, frame * elem
        if planar:
            shape, strides = (n, 3, rows, cols), (frame, step * rows, step, 1)
        elif fmt == "mono8":
            shape, strides = (n, rows, cols), (frame, step, 1)
        else:
            shape, strides = (n, rows, cols, 3), (frame, step, 3, 1)
        self.shape, self.strides, self.offset, self.total = shape, strides, offset, total
        if on_device:
            import torch
            self.backing = torch.full((total * elem,), SENTINEL, dtype=torch.uint8, device="cuda")
            self.view = torch.as_strided(self.backing.view(torch_dtype(fmt)), shape, strides, offset)

    def expected_bytes(self, converted):
        host = np.full(self.total * self.elem, SENTINEL, np.uint8)
        typed = host.view(R.bits(converted).dtype)
        dst = np.lib.stride_tricks.as_strided(typed[self.offset:], self.shape, tuple(s * self.elem for s in self.strides))
        dst[...] = R.bits(converted)
        return host

    def check(self, converted, what):
        import torch
        torch.cuda.synchronize()
        got, want = self.backing.cpu().numpy(), self.expected_bytes(converted)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: %d of %d bytes differ, the first at byte %d (row pitch %d, frame stride %d, offset %d elements)" % (
            what, bad.size, got.size, int(bad[0]), self.step_bytes, self.frame_bytes, self.offset)


def delivered(t):
    """A tensor the library returned, as the unsigned integers of its bits."""
    import torch
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return R.bits(t.cpu().numpy())


# ---- the converter's indexing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_every_format_and_width_tight(rip_lib, oracle, fmt, width):
    import torch
    h, n = 3 + width % 3, 3
    frames, e = bgr_frames(width, h, n), identity_expectation(0, width, h, n)
    pipe = plain_pipe(fmt)
    dst = Destination(fmt, n, h, width)
    with pipe.launch_log() as log:
        out = pipe.apply_device(torch.from_numpy(frames.copy()).cuda(), "bgr8", out=dst.view)
    assert out is dst.view and pipe.last_encoding == fmt
    dst.check(R.convert(e, fmt, *NORM), "%s %dx%d tight" % (fmt, width, h))
    rec = [r for r in log.records() if r["name"].startswith("output_convert_kernel")]
    assert len(rec) == 1 and rec[0]["name"] == OV.KERNEL_OF_FORMAT[fmt], log.text
    assert rec[0]["grid"] == ((width + 1023) // 1024, h) and rec[0]["block"] == 256 and rec[0]["frames"] == n and rec[0]["fc"] == 0, rec


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("width", (5, 1027))
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_pitched_and_strided_destinations(rip_lib, oracle, fmt, width, pitch):
    """Row padding, the gaps between planes and between frames and the bytes around the batch keep their sentinels; the base is
    one element off, so no row of any plane starts where the allocator's alignment would put it."""
    import torch
    h, n = 4, 3
    frames, e = bgr_frames(width, h, n, seed=1), identity_expectation(0, width, h, n, 1)
    pipe = plain_pipe(fmt)
    dst = Destination(fmt, n, h, width, pitch=pitch, gap=True, base_off=True)
    pipe.apply_device(torch.from_numpy(frames.copy()).cuda(), "bgr8", out=dst.view)
    dst.check(R.convert(e, fmt, *NORM), "%s %dx%d %s + frame gap + base offset" % (fmt, width, h, pitch))
    # the same pitches from an aligned base without a frame gap: the wide stores where the pitch allows them
    dst = Destination(fmt, n, h, width, pitch=pitch)
    pipe.apply_device(torch.from_numpy(frames.copy()).cuda(), "bgr8", out=dst.view)
    dst.check(R.convert(e, fmt, *NORM), "%s %dx%d %s" % (fmt, width, h, pitch))


def test_pitches_the_converted_geometry_cannot_hold_are_refused(rip_lib, oracle):
    import torch
    w, h, n = 8, 3, 2
    frames = torch.from_numpy(bgr_frames(w, h, n).copy()).cuda()
    pipe = plain_pipe("rgb_chw_f32")
    out = torch.full((n * 3 * h * w + 64,), 1.0, dtype=torch.float32, device="cuda")
    lib, ptr = pipe._lib, C.c_void_p

    def call(out_ptr, step, stride):
        return lib.rip_apply_device(pipe._h, ptr(frames.data_ptr()), C.c_size_t(0), C.c_size_t(0), n, h, w, 3, b"bgr8", ptr(out_ptr),
                                    C.c_size_t(step), C.c_size_t(stride), None, None)
    with pipe.launch_log() as log:
        assert call(out.data_ptr(), w * 4 - 4, 0) == P.RIP_ERR_INVALID_ARGUMENT            # a row does not fit
        assert call(out.data_ptr(), w * 4, 3 * h * w * 4 - 4) == P.RIP_ERR_INVALID_ARGUMENT  # three planes do not fit
        assert call(out.data_ptr(), w * 4 + 2, 0) == P.RIP_ERR_INVALID_ARGUMENT             # not a multiple of the element
        assert call(out.data_ptr() + 2, 0, 0) == P.RIP_ERR_INVALID_ARGUMENT
        assert call(out.data_ptr(), 1 << 24, 0) == P.RIP_ERR_INVALID_ARGUMENT               # 16 MiB per row
        torch.cuda.synchronize()
    assert not log.records() and bool((out == 1.0).all())
    assert call(out.data_ptr(), 0, 0) == P.RIP_OK
    torch.cuda.synchronize()
    got = out[:n * 3 * h * w].reshape(n, 3, h, w)
    assert np.array_equal(delivered(got), R.bits(R.convert(identity_expectation(0, w, h, n), "rgb_chw_f32", *NORM)))


# ---- the format behind the real pipeline ------------------------------------------------------------------------------------------
FULL = dict(wb=True, wb_method="grey_world", cc=True, cc_bias=(3.0, -2.0, 1.5), gamma=True, gamma_k=0.8, vig=True)
AFTER_FORMATS = ("rgb_chw_f16", "mono8", "bgr_chw_f32", "rgb8")
N_AFTER = 3


def bayer_frames(w, h, pattern, n=N_AFTER):
    return [synth.gen_frame(w, h, "bayer_%s8" % pattern, seed=300 + i, kind="uniform" if i == 1 else "scene") for i in range(n)]


def run_formats(pipe, batch, enc, expectations, what, **kw):
    """The batch under every format of AFTER_FORMATS on one handle (the format and the normalisation change between batches),
    then native again; expectations: E per frame."""
    import torch
    e = np.stack(expectations)
    for k, fmt in enumerate(AFTER_FORMATS):
        norm = NORM if k % 2 == 0 else (1.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        pipe.set_output_format(fmt)
        pipe.set_output_normalization(*norm)
        with pipe.launch_log() as log:
            out = pipe.apply_device(batch, enc, **kw)
            torch.cuda.synchronize()
        ref = R.convert(e, fmt, *norm)
        assert tuple(out.shape) == ref.shape and out.dtype == torch_dtype(fmt), (fmt, out.shape, out.dtype)
        got = delivered(out)
        assert np.array_equal(got, R.bits(ref)), "%s %s: %d of %d elements differ" % (what, fmt, int((got != R.bits(ref)).sum()), got.size)
        assert [n for n in log.names() if n.startswith("output_convert")] == [OV.KERNEL_OF_FORMAT[fmt]], log.text
    pipe.set_output_format("native")
    with pipe.launch_log() as log:
        out = pipe.apply_device(batch, enc, **kw)
        torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), e), what + ": native after the formats"
    assert not [n for n in log.names() if n.startswith("output_convert")], log.text


def test_after_the_full_chain_with_undistortion_and_a_new_image_size(rip_lib, oracle):
    import torch
    w, h = V.REMAP_SIZE
    cam = synth.camera_model(w, h)
    c = cfg(cam=cam, undistort=True, flip=True, flip_angle=180, **FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    new_size = (160, 104)
    pipe.set_undistortion_new_image_size(*new_size)
    newK = oracle.fisheye_new_camera_matrix(cam["K"], cam["D"], (w, h), cam["R"], c["balance"], new_size, c["fov_scale"])
    mx, my = oracle.fisheye_maps(cam["K"], cam["D"], cam["R"], newK, (w, h))
    frames = bayer_frames(w, h, "grbg")
    refs = []
    for f in frames:
        keep = []
        prm = oracle_params(oracle, c, keep)
        prm.map_x, prm.map_y = mx.ctypes.data, my.ctypes.data
        prm.map_rows, prm.map_cols = mx.shape
        refs.append(oracle.pipeline(prm, f, "bayer_grbg8")[0])
    run_formats(pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_grbg8", refs, "full chain + undistortion")


@pytest.mark.parametrize("fc", (0, 1))
def test_after_the_chain_under_both_contraction_models(rip_lib, oracle, fc):
    import torch
    w, h = V.CHAIN_SIZE
    c = cfg(ce=True, ce_hue=1.3, ce_sat=0.7, ce_val=1.1, **FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_fp_contraction(fc)
    frames = bayer_frames(w, h, "rggb")
    with oracle.fp_contraction(fc):
        refs = [oracle_run(oracle, c, f, "bayer_rggb8")[0] for f in frames]
    run_formats(pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_rggb8", refs, "chain fc=%d" % fc)


def test_after_flip_90(rip_lib, oracle):
    import torch
    w, h = V.CHAIN_SIZE
    c = cfg(flip=True, flip_angle=90, **FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    frames = bayer_frames(w, h, "gbrg")
    refs = [oracle_run(oracle, c, f, "bayer_gbrg8")[0] for f in frames]
    assert refs[0].shape == (w, h, 3)
    run_formats(pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_gbrg8", refs, "flip 90")


def test_after_mht(rip_lib, oracle):
    import torch
    w, h = V.CHAIN_SIZE
    c = cfg(**FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_debayer_method("mht")
    frames = bayer_frames(w, h, "bggr")
    refs = [expected_mht(oracle, c, f, "bayer_bggr8")[0] for f in frames]
    run_formats(pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_bggr8", refs, "mht")


def test_after_raw16_with_a_range_and_packed_12p(rip_lib, oracle):
    import torch
    w, h = V.CHAIN_SIZE
    c = cfg(**FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_debayer_16bit(True)
    pipe.set_debayer_16bit_range(64, 1023)
    frames = [G.gen_frame16(w, h, "rggb", 70 + i, 64, 1023, kind="random" if i == 1 else "scene") for i in range(N_AFTER)]
    refs = [expected_raw16(oracle, c, f, "rggb", "bilinear", 64, 1023)[0] for f in frames]
    batch = np.stack([np.ascontiguousarray(f, np.uint16).view(np.uint8).reshape(h, w * 2) for f in frames])
    run_formats(pipe, torch.from_numpy(batch).cuda(), G.enc16("rggb"), refs, "raw16")
    pipe.set_debayer_16bit_range(256, 4095)
    samples = [(f.astype(np.uint32) * 4).clip(0, 4095).astype(np.uint16) for f in frames]
    refs = [expected_raw16(oracle, c, f, "rggb", "bilinear", 256, 4095)[0] for f in samples]
    packed = np.stack([PKR.pack(f, "12p") for f in samples])
    run_formats(pipe, torch.from_numpy(packed).cuda(), PKR.enc("rggb", "12p"), refs, "packed 12p", width=w)


def test_ccc_sequence_keeps_its_track_and_the_taps_their_bytes(rip_lib, oracle, monkeypatch, tmp_path):
    """Five frames with temporal consistency on a handle with a format and on a native twin: the same track, the same gains, the
    same taps and the same debug dumps; the delivered tensor is the converted oracle image of every frame."""
    from helpers import DUMP_NAMES
    w, h, n = V.CHAIN_SIZE[0], V.CHAIN_SIZE[1], 5
    filt, bias = synth.ccc_model()
    c = cfg(wb=True, wb_method="ccc", wb_bright=0.8, wb_dark=0.2, wb_temporal=True, gamma=True, gamma_k=0.9)
    pipes, dirs = [], []
    for k, fmt in enumerate(("rgb_chw_bf16", "native")):
        d = tmp_path / fmt
        d.mkdir()
        monkeypatch.setenv("RIP_DEBUG_DIR", str(d))   # read when the handle is created
        p = RawImagePipeline(False, "", "", "", device=0)
        p.set_ccc_model(filt, bias)
        p.set_ccc_kalman_model(1.0, 10.0)
        configure(p, c)
        p.reset_white_balance_temporal_consistency()
        p.set_output_format(fmt)
        p.set_output_normalization(*NORM)
        p.set_debug(True)
        pipes.append(p)
        dirs.append(d)
    occ = oracle.CCC(filt, bias)
    occ.set_kalman_model(1.0, 10.0)
    for i in range(n):
        frame = synth.gen_frame(w, h, "bayer_gbrg8", seed=4100 + i, kind="scene", tint=(0.70 + 0.04 * i, 1.0, 0.55))
        ref = oracle_run(oracle, c, frame, "bayer_gbrg8", ccc=occ)[0]
        got, native = (p.process(frame, "bayer_gbrg8") for p in pipes)
        assert np.array_equal(native, ref), "native twin, frame %d" % i
        assert got.dtype == np.uint16 and np.array_equal(got, R.convert(ref, "rgb_chw_bf16", *NORM)), "frame %d" % i
        assert np.array_equal(pipes[0].get_ccc_track(1), pipes[1].get_ccc_track(1))
        assert np.array_equal(pipes[0].get_white_balance_info(1), pipes[1].get_white_balance_info(1))
        for getter in ("get_dist_debayered_image", "get_dist_color_image"):
            a, b = getattr(pipes[0], getter)(), getattr(pipes[1], getter)()
            assert a.shape == (h, w, 3) and np.array_equal(a, b), getter
        assert pipes[0].get_processed_image().size == 0 and np.array_equal(pipes[1].get_processed_image(), ref)
        for name in DUMP_NAMES:
            a, b = (d / (name + ".png")).read_bytes(), (dirs[1] / (name + ".png")).read_bytes()
            assert len(a) > 100 and a == b, name


# ---- host paths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ("rgb8", "mono8", "rgb_chw_f16"))
def test_host_paths(rip_lib, oracle, fmt):
    w, h = 37, 29
    c = cfg(**FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_output_format(fmt)
    pipe.set_output_normalization(*NORM)
    frames = bayer_frames(w, h, "rggb", 3)
    refs = [oracle_run(oracle, c, f, "bayer_rggb8")[0] for f in frames]
    want = [R.convert(e, fmt, *NORM) for e in refs]

    def same(got, k, what):
        assert got.shape == want[k].shape and got.dtype == want[k].dtype, (what, got.shape, got.dtype)
        assert np.array_equal(R.bits(got), R.bits(want[k])), "%s %s" % (fmt, what)
    same(pipe.process(frames[0], "bayer_rggb8"), 0, "process")
    assert pipe.last_encoding == fmt and pipe.get_processed_image().size == 0
    assert pipe.get_dist_debayered_image().shape == (h, w, 3)
    t = [pipe.submit(f, "bayer_rggb8") for f in frames[:2]]
    same(pipe.collect(t[0]), 0, "collect copy")
    view = pipe.collect(t[1], copy=False)
    same(view, 1, "collect view")
    assert not view.flags.writeable and pipe.get_processed_image().size == 0
    nbytes, elem, planar = pipe.query_output_bytes(h, w, 1, "bayer_rggb8")
    assert nbytes == want[0].nbytes and elem == want[0].itemsize and planar == R.is_planar(fmt)
    pinned = P.host_alloc(want[2].shape, want[2].dtype)
    pinned.view(np.uint8)[...] = SENTINEL
    got = pipe.collect(pipe.submit(frames[2], "bayer_rggb8", out=pinned))
    assert got is pinned
    same(pinned, 2, "submit into a pinned array")
    # capacities: one byte short is RIP_ERR_CAPACITY, and nothing is enqueued
    lib = pipe._lib
    small = P.host_alloc((nbytes - 1,), np.uint8)
    small[...] = SENTINEL
    ticket = C.c_uint64(0)
    f = np.ascontiguousarray(frames[0])
    with pipe.launch_log() as log:
        st = lib.rip_submit_to(pipe._h, f.ctypes.data_as(C.c_void_p), h, w, 1, C.c_size_t(w), b"bayer_rggb8", small.ctypes.data_as(C.c_void_p),
                               C.c_size_t(small.nbytes), None, None, C.c_size_t(0), C.byref(ticket))
        assert st == P.RIP_ERR_CAPACITY and ticket.value == 0
        r, cc, k = C.c_int(), C.c_int(), C.c_int()
        st = lib.rip_apply(pipe._h, f.ctypes.data_as(C.c_void_p), h, w, 1, C.c_size_t(w), b"bayer_rggb8", small.ctypes.data_as(C.c_void_p),
                           C.c_size_t(small.nbytes), C.byref(r), C.byref(cc), C.byref(k), None)
        assert st == P.RIP_ERR_CAPACITY
    assert not log.records() and (small == SENTINEL).all()
    # another normalisation and another format between frames, then native: one handle serves them all
    pipe.set_output_normalization(1.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    pipe.set_output_format("bgr_chw_f32")
    got = pipe.process(frames[1], "bayer_rggb8")
    assert got.dtype == np.float32 and np.array_equal(R.bits(got), R.bits(R.convert(refs[1], "bgr_chw_f32", 1.0)))
    assert np.array_equal(got[0], refs[1][..., 0].astype(np.float32))
    pipe.set_output_format("native")
    got = pipe.process(frames[2], "bayer_rggb8")
    assert got.dtype == np.uint8 and np.array_equal(got, refs[2]) and np.array_equal(pipe.get_processed_image(), refs[2])


def test_mono8_on_a_mono_frame_is_the_identity_without_a_kernel(rip_lib, oracle):
    w, h = 37, 29
    c = cfg(gamma=True, gamma_k=0.8)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_output_format("mono8")
    frame = synth.gen_frame(w, h, "bayer_rggb8", seed=5)
    with pipe.launch_log() as log:
        got = pipe.process(frame, "mono8")
    assert np.array_equal(got, oracle_run(oracle, c, frame, "mono8")[0].reshape(h, w)) and pipe.last_encoding == "mono8"
    assert log.names() and not [n for n in log.names() if n.startswith("output_convert")], log.text


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing_and_leave_the_state_alone(rip_lib, oracle):
    """A one-channel and a bgr16 result under a float format fail the frame call before anything is enqueued: the ccc filter of
    the handle has not moved, so the next native frames equal the oracle's sequence."""
    import torch
    w, h = V.CHAIN_SIZE
    filt, bias = synth.ccc_model()
    c = cfg(wb=True, wb_method="ccc", wb_bright=0.8, wb_dark=0.2, wb_temporal=True)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    pipe.set_ccc_model(filt, bias)
    pipe.set_ccc_kalman_model(1.0, 10.0)
    configure(pipe, c)
    pipe.reset_white_balance_temporal_consistency()
    pipe.set_debayer_16bit(True)
    occ = oracle.CCC(filt, bias)
    occ.set_kalman_model(1.0, 10.0)
    frames = [synth.gen_frame(w, h, "bayer_rggb8", seed=900 + i, tint=(0.6 + 0.1 * i, 1.0, 0.5)) for i in range(3)]
    assert np.array_equal(pipe.process(frames[0], "bayer_rggb8"), oracle_run(oracle, c, frames[0], "bayer_rggb8", ccc=occ)[0])
    pipe.set_output_format("rgb_chw_f32")
    mono = torch.from_numpy(np.stack(frames)).cuda()
    wide = torch.zeros((3, h, w * 2), dtype=torch.uint8, device="cuda")
    frame16 = frames[1].astype(np.uint16) * 257
    with pipe.launch_log() as log:
        for call in (lambda: pipe.process(frames[1], "mono8"), lambda: pipe.submit(frames[1], "mono8"), lambda: pipe.apply_device(mono, "mono8"),
                     lambda: pipe.query_output(h, w, 1, "mono8")):
            with pytest.raises(ValueError):
                call()
        # a bgr16 result exists only with every 8-bit stage off (with one on, the frame is refused whatever the format says):
        # the white balance is switched off for these calls, which leaves the ccc filter's state where it is
        pipe.set_white_balance(False)
        for call in (lambda: pipe.process(frame16, "bayer_rggb16"), lambda: pipe.submit(frame16, "bayer_rggb16"),
                     lambda: pipe.apply_device(wide, "bayer_rggb16"), lambda: pipe.query_output(h, w, 1, "bayer_rggb16")):
            with pytest.raises(ValueError):
                call()
    assert not log.records(), log.text
    pipe.set_output_format("native")
    got16 = pipe.process(frame16, "bayer_rggb16")
    assert pipe.last_encoding == "bgr16" and np.array_equal(got16, demosaic16(oracle, frame16, "rggb", "bilinear"))
    pipe.set_white_balance(True)
    for f in frames[1:]:
        assert np.array_equal(pipe.process(f, "bayer_rggb8"), oracle_run(oracle, c, f, "bayer_rggb8", ccc=occ)[0])


# ---- native is untouched, every variant runs --------------------------------------------------------------------------------------
def undistorting_pipe(w, h):
    cam = synth.camera_model(w, h)
    c = cfg(cam=cam, undistort=True, **FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    return pipe, c


def test_a_default_handle_launches_no_converter(rip_lib, oracle):
    import torch
    w, h = V.REMAP_SIZE
    frames = bayer_frames(w, h, "rggb")
    batch = torch.from_numpy(np.stack(frames)).cuda()
    logs = []
    for fmt in ("native", None, "rgb_chw_f16"):
        pipe, c = undistorting_pipe(w, h)
        if fmt is not None:
            pipe.set_output_format(fmt)
        with pipe.launch_log() as log:
            out = pipe.apply_device(batch, "bayer_rggb8")
            torch.cuda.synchronize()
        logs.append(log.text)
        if fmt != "rgb_chw_f16":
            assert "output_convert" not in log.text
            for f, o in zip(frames, out.cpu().numpy()):
                assert np.array_equal(o, oracle_run(oracle, c, f, "bayer_rggb8")[0])
    assert logs[0] == logs[1]                                   # setting "native" is the default handle, launch for launch
    lines = logs[2].splitlines()
    assert len(lines) == len(logs[0].splitlines()) + 1          # one launch more per batch slice: the converter, behind the rest
    assert [ln.split(" fc=")[0] for ln in lines if "output_convert" in ln] == ["output_convert_kernel<RgbChwF16>"] and "output_convert" in lines[-1]


@pytest.mark.parametrize("case", OV.CASES, ids=OV.case_id)
def test_every_variant_of_the_companion_runs_and_equals_the_reference(rip_lib, oracle, case):
    import torch
    w, h = case.size
    frames, e = bgr_frames(w, h, case.n_frames, seed=2), identity_expectation(0, w, h, case.n_frames, 2)
    pipe = plain_pipe(case.format, case.norm)
    with pipe.launch_log() as log:
        out = pipe.apply_device(torch.from_numpy(frames.copy()).cuda(), "bgr8")
        torch.cuda.synchronize()
    assert_launched(log, [case.name], what=case.name)
    assert (case.name, case.fc) in log.keys() and sum(n.startswith("output_convert") for n in log.names()) == 1, log.text
    assert np.array_equal(delivered(out), R.bits(R.convert(e, case.format, *case.norm)))


# ---- a seeded fuzz ----------------------------------------------------------------------------------------------------------------
FUZZ_CASES = int(os.environ.get("RIP_OUTPUT_FUZZ_CASES", "40"))
INPUT_KINDS = ("bgr8", "rgb8", "bayer8", "bayer8_mht")


def fuzz_case(seed):
    rng = np.random.default_rng(77000 + seed)
    fmt = R.FORMATS[int(rng.integers(len(R.FORMATS)))]
    norm = (float(10 ** rng.uniform(-1, 3)), tuple(float(v) for v in rng.uniform(-1, 1, 3)),
            tuple(float(v) for v in 10 ** rng.uniform(-2, 2, 3) * rng.choice([-1.0, 1.0, 1.0], 3)))
    width = int(rng.integers(3, 2101)) if rng.random() < 0.6 else int(rng.choice([3, 4, 5, 1023, 1024, 1025, 2047, 2049]))
    return dict(seed=seed, fmt=fmt, norm=norm, width=width, height=int(rng.integers(3, 10)), n=int(rng.integers(1, 6)),
                pitch=PITCHES[int(rng.integers(3))], gap=bool(rng.integers(2)), base_off=bool(rng.integers(2)),
                kind=INPUT_KINDS[int(rng.integers(len(INPUT_KINDS)))], gamma=bool(rng.integers(2)))


@pytest.mark.parametrize("seed", range(FUZZ_CASES))
def test_fuzz(rip_lib, oracle, seed):
    import torch
    k = fuzz_case(seed)
    w, h, n, fmt = k["width"], k["height"], k["n"], k["fmt"]
    c = cfg(gamma=k["gamma"], gamma_k=0.8)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    rng = np.random.default_rng(88000 + seed)
    if k["kind"] in ("bgr8", "rgb8"):
        frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        enc = k["kind"]
        e = [oracle_run(oracle, c, f, enc)[0] for f in frames]
    else:
        frames = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
        enc = "bayer_grbg8"
        if k["kind"] == "bayer8_mht":
            pipe.set_debayer_method("mht")
            e = [expected_mht(oracle, c, f, enc)[0] for f in frames]
        else:
            e = [oracle_run(oracle, c, f, enc)[0] for f in frames]
    pipe.set_output_format(fmt)
    pipe.set_output_normalization(*k["norm"])
    dst = Destination(fmt, n, h, w, pitch=k["pitch"], gap=k["gap"], base_off=k["base_off"])
    pipe.apply_device(torch.from_numpy(frames.copy()).cuda(), enc, out=dst.view)
    dst.check(R.convert(np.stack(e), fmt, *k["norm"]), str(k))


# ---- C++ facade ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade_delivers_rgb8_and_mono8(tmp_path, rip_lib, oracle, branch):
    exe = build_output_format_test(tmp_path, branch)
    w, h = 64, 48
    out_path = str(tmp_path / "out.bin")
    r = subprocess.run([exe, "gpu", str(w), str(h), out_path], capture_output=True, text=True, env=run_env(0))
    assert r.returncode == 0 and "output format gpu OK" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(out_path, np.uint8)
    assert got.size == w * h * 7
    s, vals = 12345, []
    for _ in range(w * h):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        vals.append(s >> 24)
    frame = np.array(vals, np.uint8).reshape(h, w)
    e = oracle_run(oracle, cfg(gamma=True, gamma_k=0.8), frame, "bayer_rggb8")[0]
    assert np.array_equal(got[:w * h * 3].reshape(h, w, 3), e)
    assert np.array_equal(got[w * h * 3:w * h * 6].reshape(h, w, 3), R.convert(e, "rgb8"))
    assert np.array_equal(got[w * h * 6:].reshape(h, w), R.convert(e, "mono8"))
