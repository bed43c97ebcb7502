"""The resize stage on the GPU (include/rip.h rip_set_output_size): what the frame calls deliver equals, byte for byte (float
formats as bit patterns), ``output_reference.convert(oracle.resize_linear(E, H, W), format)`` where E is the image the suite already
trusts for that input (helpers.oracle_run, expected_mht, expected_raw16) -- and not one byte outside the delivered elements is
written.

Sizes come from the kernel's constants (rip_resize.hpp: 4 output pixels per lane, 256 lanes = 1024 pixels per workgroup): output
widths 1, 3, 5, 7 end in a partial lane, 4 and 8 in a full one; 1021, 1025 and 1027 put the partial lane before, right behind and
behind a workgroup boundary, 1024 fills a workgroup exactly.  Each is paired with a source about 1.7 times as wide (a non-integer
downscale: taps at every byte offset inside a dword); 611 -> 1027 is an upscale, where the right-edge clamp is live; 2048 -> 1024
and 2050 -> 1025 with twice the rows take the 2 x 2 mean, twice the columns alone must stay linear.  Sources have 5 to 23 rows;
output heights include 1 and values above the source's rows (both rows clamp to row 0 at the top, to the last row at the bottom)."""
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
import resize_reference as Z
import resize_variant_cases as RV
import variant_cases as V
from helpers import cfg, configure, expected_mht, oracle_params, oracle_run
from raw16_reference import demosaic16, expected_raw16
from raw_image_pipeline_amd import RawImagePipeline, synth
from raw_image_pipeline_amd import pipeline as P
from test_cpp_facade import BRANCHES, run_env
from test_output_format_gpu import FULL, NORM, PITCHES, SENTINEL, Destination, bayer_frames, delivered
from test_resize import build_resize_test

pytestmark = pytest.mark.gpu

OUT_WIDTHS = (1, 3, 4, 5, 7, 8, 1021, 1024, 1025, 1027)
LAYOUT_OF = {"native3": "rgb8", "native1": "mono8"}     # Destination's layouts of the two native results: interleaved bytes


def src_width(w):
    return max(3, (w * 17 + 5) // 10)                   # about 1.7 x (3 x for one pixel), never twice the target


@functools.lru_cache(maxsize=None)
def noise(w, h, n, cn, seed=0):
    """n frames of uniform noise (every byte value, every neighbourhood: one wrong tap or weight shows).  Shared; read-only."""
    f = np.random.default_rng(4000 + seed + 7 * w + 13 * h + cn).integers(0, 256, (n, h, w) if cn == 1 else (n, h, w, 3), dtype=np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def trusted(w, h, n, cn, seed=0):
    """E of noise(...) under a configuration with every stage off, from the oracle.  Shared; read-only."""
    import oracle as O
    enc = "mono8" if cn == 1 else "bgr8"
    e = np.stack([oracle_run(O, cfg(), np.ascontiguousarray(f), enc)[0].reshape(f.shape) for f in noise(w, h, n, cn, seed)])
    e.setflags(write=False)
    return e


def resized(O, e, H, W):
    """oracle.resize_linear on every frame of a stack."""
    return np.stack([O.resize_linear(np.ascontiguousarray(f), H, W) for f in e])


def want(O, e, H, W, fmt):
    """What a handle with target (W, H) and format fmt delivers for the trusted frames e."""
    r = resized(O, e, H, W)
    if fmt in ("native", "native1", "native3") or (fmt == "mono8" and r.ndim == 3):
        return r
    return R.convert(r, fmt, *NORM)


def plain_pipe(target, fmt="native"):
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, cfg())
    pipe.set_output_format(fmt)
    pipe.set_output_normalization(*NORM)
    if target is not None:
        pipe.set_output_size(*target)
    return pipe


def apply_into(pipe, frames, enc, view):
    """rip_apply_device with the destination given as a strided view (row pitch and frame stride from its strides): the C call
    itself, because RawImagePipeline.apply_device takes native results only as contiguous tensors."""
    import torch
    n, rows, cols = frames.shape[:3]
    cn = 1 if frames.dim() == 3 else frames.shape[3]
    elem = view.element_size()
    planar = view.dim() == 4 and view.shape[1] == 3 and view.stride(3) == 1 and view.dtype != torch.uint8
    step = view.stride(2 if planar else 1) * elem
    frame = view.stride(0) * elem
    st = pipe._lib.rip_apply_device(pipe._h, C.c_void_p(frames.data_ptr()), C.c_size_t(0), C.c_size_t(0), int(n), int(rows), int(cols), int(cn),
                                    enc.encode(), C.c_void_p(view.data_ptr()), C.c_size_t(step), C.c_size_t(frame), None, None)
    pipe._check(st)
    torch.cuda.synchronize()


def resize_records(log):
    return [r for r in log.records() if r["name"].startswith("resize_kernel")]


def run_case(O, cn, src, dst, fmt, n=2, pitch="tight", gap=False, base_off=False, seed=0):
    """noise frames of src = (w, h) resized to dst = (w, h) under fmt into a sentinel-filled destination; returns the launch log."""
    import torch
    (sw, sh), (dw, dh) = src, dst
    frames, e = noise(sw, sh, n, cn, seed), trusted(sw, sh, n, cn, seed)
    pipe = plain_pipe((dw, dh), "native" if fmt.startswith("native") else fmt)
    d = Destination(LAYOUT_OF.get(fmt, fmt), n, dh, dw, pitch=pitch, gap=gap, base_off=base_off)
    with pipe.launch_log() as log:
        apply_into(pipe, torch.from_numpy(frames.copy()).cuda(), "mono8" if cn == 1 else "bgr8", d.view)
    d.check(want(O, e, dh, dw, fmt), "%s %dx%dx%d -> %dx%d %s" % (fmt, sw, sh, cn, dw, dh, pitch))
    return log


# ---- the kernel's indexing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", (1, 3))
@pytest.mark.parametrize("width", OUT_WIDTHS)
def test_every_width_downscaled_native(rip_lib, oracle, width, cn):
    sh, dh = 9 + width % 3, 5
    log = run_case(oracle, cn, (src_width(width), sh), (width, dh), "native%d" % cn)
    rec = resize_records(log)
    assert len(rec) == 1 and rec[0]["name"] == RV.kernel_name(cn, False), log.text
    assert rec[0]["grid"] == ((width + 1023) // 1024, dh) and rec[0]["block"] == 256 and rec[0]["frames"] == 2 and rec[0]["fc"] == 0, rec
    assert "output_convert" not in log.text


@pytest.mark.parametrize("cn", (1, 3))
@pytest.mark.parametrize("src,dst", (((611, 5), (1027, 9)),      # upscale on both axes: right-edge and bottom clamps, sy = -1 at the top
                                     ((1747, 23), (1027, 1)),    # one output row
                                     ((7, 6), (1024, 40)),       # a source narrower than one lane's span, far more rows out than in
                                     ((1, 1), (5, 3)),           # a one-pixel source: every tap is that pixel
                                     ((1747, 5), (1, 7))))       # one output column
def test_upscales_and_extreme_heights(rip_lib, oracle, src, dst, cn):
    log = run_case(oracle, cn, src, dst, "native%d" % cn, seed=1)
    assert [r["name"] for r in resize_records(log)] == [RV.kernel_name(cn, False)], log.text


@pytest.mark.parametrize("cn", (1, 3))
@pytest.mark.parametrize("sw,dw", ((2048, 1024), (2050, 1025), (14, 7), (2, 1)))
def test_exactly_half_on_both_axes_is_the_2x2_mean(rip_lib, oracle, sw, dw, cn):
    dh = 5
    log = run_case(oracle, cn, (sw, 2 * dh), (dw, dh), "native%d" % cn, seed=2)
    assert [r["name"] for r in resize_records(log)] == [RV.kernel_name(cn, True)], log.text


@pytest.mark.parametrize("cn", (1, 3))
def test_half_on_one_axis_only_stays_linear(rip_lib, oracle, cn):
    for src, dst in (((2050, 9), (1025, 5)), ((1747, 10), (1027, 5)), ((2050, 10), (1025, 10))):
        log = run_case(oracle, cn, src, dst, "native%d" % cn, seed=3)
        assert [r["name"] for r in resize_records(log)] == [RV.kernel_name(cn, False)], log.text


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_every_format_behind_the_resize(rip_lib, oracle, fmt):
    """The converter runs unchanged on F': exactly one resize launch in front of exactly one converter launch."""
    for src, dst, area in (((1747, 9), (1027, 5), False), ((2050, 10), (1025, 5), True)):
        log = run_case(oracle, 3, src, dst, fmt, n=3)
        names = [n for n in log.names() if n.startswith(("resize_kernel", "output_convert"))]
        assert names == [RV.kernel_name(3, area), OV.KERNEL_OF_FORMAT[fmt]], log.text
        assert log.names()[-2:] == names


def test_mono8_on_a_one_channel_result_stays_the_identity_on_the_resized_image(rip_lib, oracle):
    log = run_case(oracle, 1, (1747, 9), (1027, 5), "mono8")
    assert [r["name"] for r in resize_records(log)] == [RV.kernel_name(1, False)] and "output_convert" not in log.text


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("width", (5, 1027))
@pytest.mark.parametrize("fmt", ("native3", "native1", "rgb8", "mono8", "rgb_chw_f16", "bgr_chw_f32"))
def test_pitched_and_strided_destinations(rip_lib, oracle, fmt, width, pitch):
    """Row padding, the gaps between planes and between frames and the bytes around the batch keep their sentinels; the base is
    one element off, so no row starts where the allocator's alignment would put it -- then the same pitches from an aligned base,
    where the dword stores are taken."""
    cn = 1 if fmt == "native1" else 3
    src, dst = (src_width(width), 9), (width, 5)
    run_case(oracle, cn, src, dst, fmt, n=3, pitch=pitch, gap=True, base_off=True, seed=4)
    run_case(oracle, cn, src, dst, fmt, n=3, pitch=pitch, seed=4)
    run_case(oracle, cn, (2 * width, 10), dst, fmt, n=3, pitch=pitch, gap=True, base_off=True, seed=4)     # the 2 x 2 path's stores


def test_pitches_the_delivered_geometry_cannot_hold_are_refused(rip_lib, oracle):
    import torch
    sw, sh, w, h, n = 14, 9, 8, 5, 2
    frames = torch.from_numpy(noise(sw, sh, n, 3).copy()).cuda()
    pipe = plain_pipe((w, h))
    out = torch.full((n * h * w * 3 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")

    def call(step, stride):
        return pipe._lib.rip_apply_device(pipe._h, C.c_void_p(frames.data_ptr()), C.c_size_t(0), C.c_size_t(0), n, sh, sw, 3, b"bgr8",
                                          C.c_void_p(out.data_ptr()), C.c_size_t(step), C.c_size_t(stride), None, None)
    with pipe.launch_log() as log:
        assert call(w * 3 - 1, 0) == P.RIP_ERR_INVALID_ARGUMENT                    # a delivered row does not fit
        assert call(w * 3, h * w * 3 - 1) == P.RIP_ERR_INVALID_ARGUMENT            # a delivered frame does not fit
        assert call(1 << 24, 0) == P.RIP_ERR_INVALID_ARGUMENT
        torch.cuda.synchronize()
    assert not log.records() and bool((out == SENTINEL).all())
    assert call(w * 3, h * w * 3) == P.RIP_OK                                      # tight for the delivered size, too small for F's
    torch.cuda.synchronize()
    got = out[:n * h * w * 3].reshape(n, h, w, 3).cpu().numpy()
    assert np.array_equal(got, resized(oracle, trusted(sw, sh, n, 3), h, w)) and bool((out[n * h * w * 3:] == SENTINEL).all())


# ---- the resize behind the real pipeline -----------------------------------------------------------------------------------------
AFTER_FORMATS = ("native", "rgb_chw_f16", "mono8")


def run_resized(O, pipe, batch, enc, expectations, what, targets=None, **kw):
    """The batch under every format of AFTER_FORMATS and two targets on one handle (target and format change between batches),
    then without a target again; expectations: E per frame."""
    import torch
    e = np.stack(expectations)
    rows, cols = e.shape[1:3]
    targets = targets or ((max(1, cols * 10 // 17), max(1, rows * 10 // 17)), (cols + cols // 3, rows + 3))
    for k, fmt in enumerate(AFTER_FORMATS):
        w, h = targets[k % len(targets)]
        pipe.set_output_format(fmt)
        pipe.set_output_normalization(*NORM)
        pipe.set_output_size(w, h)
        with pipe.launch_log() as log:
            out = pipe.apply_device(batch, enc, **kw)
            torch.cuda.synchronize()
        ref = want(O, e, h, w, fmt)
        assert tuple(out.shape) == ref.shape, (what, fmt, out.shape, ref.shape)
        got = delivered(out)
        assert np.array_equal(got, R.bits(ref)), "%s %s -> %dx%d: %d of %d elements differ" % (what, fmt, w, h, int((got != R.bits(ref)).sum()), got.size)
        tail = [n for n in log.names() if n.startswith(("resize_kernel", "output_convert"))]
        assert tail == [RV.kernel_name(3, False)] + ([OV.KERNEL_OF_FORMAT[fmt]] if fmt != "native" else []) and log.names()[-len(tail):] == tail, log.text
    pipe.set_output_format("native")
    for target in ((cols, rows), (0, 0)):          # F's own size, and no target: the frames as without the stage
        pipe.set_output_size(*target)
        with pipe.launch_log() as log:
            out = pipe.apply_device(batch, enc, **kw)
            torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), e), "%s: target %s" % (what, target)
        assert "resize_kernel" not in log.text and "output_convert" not in log.text, log.text


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
    run_resized(oracle, pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_grbg8", refs, "full chain + undistortion")
    # the camera matrix of what was delivered last with a target
    rows, cols = refs[0].shape[:2]
    pipe.set_output_size(64, 40)
    hh, ww, k, pr = pipe.get_output_camera_info(h, w, 1, "bayer_grbg8")
    wk, wp = Z.scaled_camera(pipe.get_rect_camera_matrix(), pipe.get_rect_projection_matrix(), rows, cols, 40, 64)
    assert (hh, ww) == (40, 64) and np.array_equal(k, wk) and np.array_equal(pr, wp)


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
    run_resized(oracle, pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_rggb8", refs, "chain fc=%d" % fc)


def test_after_flip_90(rip_lib, oracle):
    import torch
    w, h = V.CHAIN_SIZE
    c = cfg(flip=True, flip_angle=90, **FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    frames = bayer_frames(w, h, "gbrg")
    refs = [oracle_run(oracle, c, f, "bayer_gbrg8")[0] for f in frames]
    assert refs[0].shape == (w, h, 3)
    run_resized(oracle, pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_gbrg8", refs, "flip 90")


def test_after_mht(rip_lib, oracle):
    import torch
    w, h = V.CHAIN_SIZE
    c = cfg(**FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_debayer_method("mht")
    frames = bayer_frames(w, h, "bggr")
    refs = [expected_mht(oracle, c, f, "bayer_bggr8")[0] for f in frames]
    run_resized(oracle, pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_bggr8", refs, "mht")


def test_after_raw16_with_a_range_and_packed_12p(rip_lib, oracle):
    import torch
    w, h = V.CHAIN_SIZE
    c = cfg(**FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_debayer_16bit(True)
    pipe.set_debayer_16bit_range(64, 1023)
    frames = [G.gen_frame16(w, h, "rggb", 70 + i, 64, 1023, kind="random" if i == 1 else "scene") for i in range(3)]
    refs = [expected_raw16(oracle, c, f, "rggb", "bilinear", 64, 1023)[0] for f in frames]
    batch = np.stack([np.ascontiguousarray(f, np.uint16).view(np.uint8).reshape(h, w * 2) for f in frames])
    run_resized(oracle, pipe, torch.from_numpy(batch).cuda(), G.enc16("rggb"), refs, "raw16")
    pipe.set_debayer_16bit_range(256, 4095)
    samples = [(f.astype(np.uint32) * 4).clip(0, 4095).astype(np.uint16) for f in frames]
    refs = [expected_raw16(oracle, c, f, "rggb", "bilinear", 256, 4095)[0] for f in samples]
    packed = np.stack([PKR.pack(f, "12p") for f in samples])
    run_resized(oracle, pipe, torch.from_numpy(packed).cuda(), PKR.enc("rggb", "12p"), refs, "packed 12p", width=w)


def test_ccc_sequence_keeps_its_track_and_the_taps_their_bytes(rip_lib, oracle, monkeypatch, tmp_path):
    """Five frames with temporal consistency on a handle with a target and on a twin without: the same track, the same gains, the
    same taps and the same debug dumps; the delivered frame is the resized oracle image of every frame."""
    from helpers import DUMP_NAMES
    w, h, n = V.CHAIN_SIZE[0], V.CHAIN_SIZE[1], 5
    tw, th = w * 10 // 17, h * 10 // 17
    filt, bias = synth.ccc_model()
    c = cfg(wb=True, wb_method="ccc", wb_bright=0.8, wb_dark=0.2, wb_temporal=True, gamma=True, gamma_k=0.9)
    pipes, dirs = [], []
    for target in ((tw, th), (0, 0)):
        d = tmp_path / ("t%d" % target[0])
        d.mkdir()
        monkeypatch.setenv("RIP_DEBUG_DIR", str(d))   # read when the handle is created
        p = RawImagePipeline(False, "", "", "", device=0)
        p.set_ccc_model(filt, bias)
        p.set_ccc_kalman_model(1.0, 10.0)
        configure(p, c)
        p.reset_white_balance_temporal_consistency()
        p.set_output_size(*target)
        p.set_debug(True)
        pipes.append(p)
        dirs.append(d)
    occ = oracle.CCC(filt, bias)
    occ.set_kalman_model(1.0, 10.0)
    for i in range(n):
        frame = synth.gen_frame(w, h, "bayer_gbrg8", seed=4100 + i, kind="scene", tint=(0.70 + 0.04 * i, 1.0, 0.55))
        ref = oracle_run(oracle, c, frame, "bayer_gbrg8", ccc=occ)[0]
        got, twin = (p.process(frame, "bayer_gbrg8") for p in pipes)
        assert np.array_equal(twin, ref), "twin without a target, frame %d" % i
        assert got.shape == (th, tw, 3) and np.array_equal(got, oracle.resize_linear(ref, th, tw)), "frame %d" % i
        assert pipes[0].last_encoding == "bgr8"
        assert np.array_equal(pipes[0].get_ccc_track(1), pipes[1].get_ccc_track(1))
        assert np.array_equal(pipes[0].get_white_balance_info(1), pipes[1].get_white_balance_info(1))
        for getter in ("get_dist_debayered_image", "get_dist_color_image"):
            a, b = getattr(pipes[0], getter)(), getattr(pipes[1], getter)()
            assert a.shape == (h, w, 3) and np.array_equal(a, b), getter
        assert pipes[0].get_processed_image().size == 0 and np.array_equal(pipes[1].get_processed_image(), ref)
        for name in DUMP_NAMES:
            a, b = (dirs[0] / (name + ".png")).read_bytes(), (dirs[1] / (name + ".png")).read_bytes()
            assert len(a) > 100 and a == b, name


# ---- host paths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ("native", "rgb8", "rgb_chw_f16"))
def test_host_paths(rip_lib, oracle, fmt):
    w, h, tw, th = 37, 29, 21, 17
    c = cfg(**FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_output_format(fmt)
    pipe.set_output_normalization(*NORM)
    pipe.set_output_size(tw, th)
    frames = bayer_frames(w, h, "rggb", 3)
    refs = [oracle_run(oracle, c, f, "bayer_rggb8")[0] for f in frames]
    wants = [want(oracle, e[None], th, tw, fmt)[0] for e in refs]
    enc = "bgr8" if fmt == "native" else fmt

    def same(got, k, what):
        assert got.shape == wants[k].shape and got.dtype == wants[k].dtype, (what, got.shape, got.dtype)
        assert np.array_equal(R.bits(got), R.bits(wants[k])), "%s %s" % (fmt, what)
    same(pipe.process(frames[0], "bayer_rggb8"), 0, "process")
    assert pipe.last_encoding == enc and pipe.get_processed_image().size == 0
    assert pipe.get_dist_debayered_image().shape == (h, w, 3) and pipe.get_dist_color_image().shape == (h, w, 3)
    t = [pipe.submit(f, "bayer_rggb8") for f in frames[:2]]
    same(pipe.collect(t[0]), 0, "collect copy")
    view = pipe.collect(t[1], copy=False)
    same(view, 1, "collect view")
    assert not view.flags.writeable and pipe.get_processed_image().size == 0
    nbytes, elem, planar = pipe.query_output_bytes(h, w, 1, "bayer_rggb8")
    assert nbytes == wants[0].nbytes and elem == wants[0].itemsize and planar == (fmt == "rgb_chw_f16")
    pinned = P.host_alloc(wants[2].shape, wants[2].dtype)
    pinned.view(np.uint8)[...] = SENTINEL
    got = pipe.collect(pipe.submit(frames[2], "bayer_rggb8", out=pinned))
    assert got is pinned
    same(pinned, 2, "submit into a pinned array")
    # capacities are the delivered frame's: one byte short is RIP_ERR_CAPACITY, and nothing is enqueued
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
    # another target between frames, then none: one handle serves them all
    pipe.set_output_size(74, 58)
    got = pipe.process(frames[1], "bayer_rggb8")
    assert np.array_equal(R.bits(got), R.bits(want(oracle, refs[1][None], 58, 74, fmt)[0]))
    pipe.set_output_size(0, 0)
    pipe.set_output_format("native")
    got = pipe.process(frames[2], "bayer_rggb8")
    assert got.dtype == np.uint8 and np.array_equal(got, refs[2]) and np.array_equal(pipe.get_processed_image(), refs[2])


def test_a_mono_frame_through_the_host_paths(rip_lib, oracle):
    w, h, tw, th = 37, 29, 64, 11
    c = cfg(gamma=True, gamma_k=0.8)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_output_size(tw, th)
    frame = synth.gen_frame(w, h, "bayer_rggb8", seed=5)
    ref = oracle.resize_linear(np.ascontiguousarray(oracle_run(oracle, c, frame, "mono8")[0].reshape(h, w)), th, tw)
    for fmt in ("native", "mono8"):
        pipe.set_output_format(fmt)
        with pipe.launch_log() as log:
            got = pipe.process(frame, "mono8")
        assert got.shape == (th, tw) and np.array_equal(got, ref) and pipe.last_encoding == "mono8"
        assert [r["name"] for r in resize_records(log)] == [RV.kernel_name(1, False)] and "output_convert" not in log.text
        assert np.array_equal(pipe.collect(pipe.submit(frame, "mono8")), ref)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing_and_leave_the_state_alone(rip_lib, oracle):
    """A bgr16 result under a target, and a one-channel result under a float format with a target, fail the frame call before
    anything is enqueued: the ccc filter of the handle has not moved, so the next frames equal the oracle's sequence."""
    import torch
    w, h = V.CHAIN_SIZE
    tw, th = w // 2 + 3, h // 2 + 1
    filt, bias = synth.ccc_model()
    c = cfg(wb=True, wb_method="ccc", wb_bright=0.8, wb_dark=0.2, wb_temporal=True)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    pipe.set_ccc_model(filt, bias)
    pipe.set_ccc_kalman_model(1.0, 10.0)
    configure(pipe, c)
    pipe.reset_white_balance_temporal_consistency()
    pipe.set_debayer_16bit(True)
    pipe.set_output_size(tw, th)
    occ = oracle.CCC(filt, bias)
    occ.set_kalman_model(1.0, 10.0)
    frames = [synth.gen_frame(w, h, "bayer_rggb8", seed=900 + i, tint=(0.6 + 0.1 * i, 1.0, 0.5)) for i in range(3)]

    def expect(f):
        return oracle.resize_linear(oracle_run(oracle, c, f, "bayer_rggb8", ccc=occ)[0], th, tw)
    assert np.array_equal(pipe.process(frames[0], "bayer_rggb8"), expect(frames[0]))
    mono = torch.from_numpy(np.stack(frames)).cuda()
    wide = torch.zeros((3, h, w * 2), dtype=torch.uint8, device="cuda")
    frame16 = frames[1].astype(np.uint16) * 257
    with pipe.launch_log() as log:
        pipe.set_output_format("rgb_chw_f32")
        for call in (lambda: pipe.process(frames[1], "mono8"), lambda: pipe.submit(frames[1], "mono8"), lambda: pipe.apply_device(mono, "mono8"),
                     lambda: pipe.query_output(h, w, 1, "mono8")):
            with pytest.raises(ValueError):
                call()
        pipe.set_output_format("native")
        # a bgr16 result exists only with every 8-bit stage off: the white balance is switched off for these calls, which leaves
        # the ccc filter's state where it is
        pipe.set_white_balance(False)
        for call in (lambda: pipe.process(frame16, "bayer_rggb16"), lambda: pipe.submit(frame16, "bayer_rggb16"),
                     lambda: pipe.apply_device(wide, "bayer_rggb16"), lambda: pipe.query_output(h, w, 1, "bayer_rggb16")):
            with pytest.raises(ValueError):
                call()
    assert not log.records(), log.text
    pipe.set_output_size(0, 0)
    got16 = pipe.process(frame16, "bayer_rggb16")
    assert pipe.last_encoding == "bgr16" and np.array_equal(got16, demosaic16(oracle, frame16, "rggb", "bilinear"))
    pipe.set_output_size(tw, th)
    pipe.set_white_balance(True)
    for f in frames[1:]:
        assert np.array_equal(pipe.process(f, "bayer_rggb8"), expect(f))


# ---- without a target nothing changes, every variant runs ------------------------------------------------------------------------
def undistorting_pipe(w, h):
    cam = synth.camera_model(w, h)
    c = cfg(cam=cam, undistort=True, **FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    return pipe, c


def test_a_default_handle_and_a_target_of_the_images_own_size_launch_no_resize(rip_lib, oracle):
    import torch
    w, h = V.REMAP_SIZE
    frames = bayer_frames(w, h, "rggb")
    batch = torch.from_numpy(np.stack(frames)).cuda()
    logs = {}
    for fmt in ("native", "rgb_chw_f16"):
        for target in (None, (0, 0), (w, h), (w // 2 + 1, h // 2 + 1)):
            pipe, c = undistorting_pipe(w, h)
            pipe.set_output_format(fmt)
            if target is not None:
                pipe.set_output_size(*target)
            with pipe.launch_log() as log:
                out = pipe.apply_device(batch, "bayer_rggb8")
                torch.cuda.synchronize()
            logs[fmt, target] = log.text
            if fmt == "native" and target != (w // 2 + 1, h // 2 + 1):
                for f, o in zip(frames, out.cpu().numpy()):
                    assert np.array_equal(o, oracle_run(oracle, c, f, "bayer_rggb8")[0])
        assert logs[fmt, None] == logs[fmt, (0, 0)] == logs[fmt, (w, h)] and "resize_kernel" not in logs[fmt, None]
        base, active = logs[fmt, None].splitlines(), logs[fmt, (w // 2 + 1, h // 2 + 1)].splitlines()
        assert len(active) == len(base) + 1                         # one launch more per batch slice
        at = [i for i, ln in enumerate(active) if ln.startswith("resize_kernel")]
        assert len(at) == 1 and active[at[0]].split(" fc=")[0] == RV.kernel_name(3, False)
        if fmt == "native":
            assert at[0] == len(active) - 1                         # behind the pipeline's last kernel
        else:
            assert at[0] == len(active) - 2 and active[-1].startswith("output_convert_kernel<RgbChwF16>")   # in front of the converter
    assert "output_convert" not in logs["native", (w // 2 + 1, h // 2 + 1)]


@pytest.mark.parametrize("case", RV.CASES, ids=RV.case_id)
def test_every_variant_of_the_companion_runs_and_equals_the_oracle(rip_lib, oracle, case):
    import torch
    (sw, sh), (dw, dh) = case.src_size, case.dst_size
    frames, e = noise(sw, sh, case.n_frames, case.channels, seed=5), trusted(sw, sh, case.n_frames, case.channels, 5)
    pipe = plain_pipe((dw, dh))
    with pipe.launch_log() as log:
        out = pipe.apply_device(torch.from_numpy(frames.copy()).cuda(), case.encoding)
        torch.cuda.synchronize()
    assert (case.name, case.fc) in log.keys() and sum(n.startswith("resize_kernel") for n in log.names()) == 1, log.text
    assert np.array_equal(out.cpu().numpy(), resized(oracle, e, dh, dw))


# ---- a seeded fuzz ----------------------------------------------------------------------------------------------------------------
FUZZ_CASES = int(os.environ.get("RIP_RESIZE_FUZZ_CASES", "40"))
FUZZ_FORMATS = ("native",) + R.FORMATS


def fuzz_case(seed):
    rng = np.random.default_rng(99000 + seed)
    cn = int(rng.choice([1, 3]))
    fmt = FUZZ_FORMATS[int(rng.integers(len(FUZZ_FORMATS)))] if cn == 3 else ("native", "mono8")[int(rng.integers(2))]
    sw, sh, dw, dh = (int(v) for v in rng.integers(1, 71, 4))
    if rng.random() < 0.15:
        sw, sh = 2 * dw, 2 * dh                                      # the 2 x 2 switch
    elif rng.random() < 0.1:
        sw = 2 * dw                                                  # 2 x on one axis only
    return dict(seed=seed, cn=cn, fmt=fmt, src=(sw, sh), dst=(dw, dh), n=int(rng.integers(1, 6)), pitch=PITCHES[int(rng.integers(3))],
                gap=bool(rng.integers(2)), base_off=bool(rng.integers(2)))


@pytest.mark.parametrize("seed", range(FUZZ_CASES))
def test_fuzz(rip_lib, oracle, seed):
    k = fuzz_case(seed)
    fmt = "native%d" % k["cn"] if k["fmt"] == "native" else k["fmt"]
    log = run_case(oracle, k["cn"], k["src"], k["dst"], fmt, n=k["n"], pitch=k["pitch"], gap=k["gap"], base_off=k["base_off"], seed=100 + seed)
    area = k["src"] == (2 * k["dst"][0], 2 * k["dst"][1])
    expect = [] if k["src"] == k["dst"] else [RV.kernel_name(k["cn"], area)]      # a target of F's own size launches nothing
    assert [r["name"] for r in resize_records(log)] == expect, (k, log.text)


# ---- C++ facade ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade_delivers_resized_frames(tmp_path, rip_lib, oracle, branch):
    exe = build_resize_test(tmp_path, branch)
    w, h, tw, th = 64, 48, 37, 29
    out_path = str(tmp_path / "out.bin")
    r = subprocess.run([exe, "gpu", str(w), str(h), str(tw), str(th), out_path], capture_output=True, text=True, env=run_env(0))
    assert r.returncode == 0 and "resize gpu OK" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(out_path, np.uint8)
    assert got.size == w * h * 3 + 2 * tw * th * 3
    s, vals = 12345, []
    for _ in range(w * h):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        vals.append(s >> 24)
    frame = np.array(vals, np.uint8).reshape(h, w)
    e = oracle_run(oracle, cfg(gamma=True, gamma_k=0.8), frame, "bayer_rggb8")[0]
    small = oracle.resize_linear(e, th, tw)
    assert np.array_equal(got[:w * h * 3].reshape(h, w, 3), e)
    assert np.array_equal(got[w * h * 3:w * h * 3 + tw * th * 3].reshape(th, tw, 3), small)
    assert np.array_equal(got[w * h * 3 + tw * th * 3:].reshape(th, tw, 3), R.convert(small, "rgb8"))
