"""The resize stage under the "area" interpolation on the GPU (include/rip.h rip_set_output_interpolation): what the frame calls
deliver equals, byte for byte (float formats as bit patterns), ``output_reference.convert(area_reference.resize(E, H, W), format)``
where E is the image the suite already trusts for that input (helpers.oracle_run, expected_mht, expected_raw16) -- and not one byte
outside the delivered elements is written.  Tolerance 0 everywhere.

Sizes come from the launch code (rip_area.hpp: a workgroup owns 64 x 8 output pixels, one lane per output column, four waves that
take the rows w, w + 4 of the rectangle): tests/area_cases.py lists target widths 63 / 64 / 65 / 133 and heights 7 / 8 / 9 / 19, and
the factors at which the tap lists change shape.  Sources stay below about 300 x 300 apart from one 2051 x 5 strip."""
import ctypes as C
import functools

import numpy as np
import pytest

import area_cases as AC
import area_reference as A
import area_variant_cases as AV
import output_reference as R
import output_variant_cases as OV
import packed_reference as PKR
import raw16_cases as G
import variant_cases as V
from helpers import cfg, configure, expected_mht, oracle_params, oracle_run
from raw16_reference import expected_raw16
from raw_image_pipeline_amd import RawImagePipeline, synth
from raw_image_pipeline_amd import pipeline as P
from test_output_format_gpu import FULL, NORM, PITCHES, SENTINEL, Destination, bayer_frames, delivered, torch_dtype
from test_resize_gpu import LAYOUT_OF, apply_into, noise, trusted

pytestmark = pytest.mark.gpu

KERNELS = ("area_reduce_kernel", "resize_kernel", "output_convert")


def want(e, H, W, fmt):
    """What a handle with target (W, H), "area" and format fmt delivers for the trusted frames e."""
    r = A.resize_stack(e, H, W)
    if fmt in ("native", "native1", "native3") or (fmt == "mono8" and r.ndim == 3):
        return r
    return R.convert(r, fmt, *NORM)


def area_pipe(target, fmt="native", interpolation="area"):
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, cfg())
    pipe.set_output_format(fmt)
    pipe.set_output_normalization(*NORM)
    pipe.set_output_interpolation(interpolation)
    if target is not None:
        pipe.set_output_size(*target)
    return pipe


def destination(fmt, n, rows, cols, pitch="tight", gap=False, offset=0):
    """test_output_format_gpu.Destination with the base `offset` elements (not only 0 or 1) into the buffer."""
    import torch
    d = Destination(fmt, n, rows, cols, pitch=pitch, gap=gap, base_off=False, on_device=False)
    d.offset, d.total = offset, d.total + offset
    d.backing = torch.full((d.total * d.elem,), SENTINEL, dtype=torch.uint8, device="cuda")
    d.view = torch.as_strided(d.backing.view(torch_dtype(fmt)), d.shape, d.strides, d.offset)
    return d


@functools.lru_cache(maxsize=None)
def trusted_of(key):
    """E of the crafted frames of tests/area_cases.py under a configuration with every stage off, from the oracle.  Read-only."""
    import oracle as O
    name, cn = key
    f = AC.tie_frame(cn) if name == "ties" else AC.all_255({"flat512": (512, 256), "flat153": (153, 128)}[name], cn)
    e = oracle_run(O, cfg(), np.ascontiguousarray(f), "mono8" if cn == 1 else "bgr8")[0].reshape(f.shape)
    assert np.array_equal(e, f)                      # every stage off: F is the input, so the crafted sums reach the resize
    f.setflags(write=False)
    return f[None]


def records(log):
    return [r for r in log.records() if r["name"].startswith(KERNELS[:2])]


def run_case(cn, src, dst, fmt, n=2, pitch="tight", gap=False, offset=0, seed=0, frames=None, pipe=None):
    """Frames of src = (w, h) -- noise unless given -- resized to dst = (w, h) under fmt into a sentinel-filled destination."""
    import torch
    (sw, sh), (dw, dh) = src, dst
    if frames is None:
        frames, e = noise(sw, sh, n, cn, seed), trusted(sw, sh, n, cn, seed)
    else:
        e, n = frames, len(frames)
    pipe = pipe or area_pipe((dw, dh), "native" if fmt.startswith("native") else fmt)
    d = destination(LAYOUT_OF.get(fmt, fmt), n, dh, dw, pitch=pitch, gap=gap, offset=offset)
    with pipe.launch_log() as log:
        apply_into(pipe, torch.from_numpy(np.array(frames)).cuda(), "mono8" if cn == 1 else "bgr8", d.view)
    d.check(want(e, dh, dw, fmt), "%s %dx%dx%d -> %dx%d %s offset %d" % (fmt, sw, sh, cn, dw, dh, pitch, offset))
    return log


def assert_one_launch(log, cn, src, dst, n):
    kind = AC.kind_of(src, dst)
    rec = records(log)
    assert [r["name"] for r in rec] == [AC.kernel_name(cn, kind)], log.text
    if kind != "mean2":
        grid = ((dst[0] + AC.TILE_W - 1) // AC.TILE_W, (dst[1] + AC.TILE_H - 1) // AC.TILE_H)
        assert rec[0]["grid"] == grid and rec[0]["block"] == 256 and rec[0]["frames"] == n and rec[0]["fc"] == 0, rec


# ---- the kernel's indexing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", (1, 3))
@pytest.mark.parametrize("shape", AC.SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s.src + s.dst))
def test_tile_edges_and_factors_native(rip_lib, oracle, shape, cn):
    log = run_case(cn, shape.src, shape.dst, "native%d" % cn)
    assert_one_launch(log, cn, shape.src, shape.dst, 2)
    assert "output_convert" not in log.text


@pytest.mark.parametrize("cn", (1, 3))
def test_exactly_half_on_both_axes_equals_a_linear_handles_frame(rip_lib, oracle, cn):
    import torch
    src, dst = (30, 20), (15, 10)
    frames = torch.from_numpy(noise(*src, 2, cn).copy()).cuda()
    outs = []
    for name in ("area", "linear"):
        pipe = area_pipe(dst, interpolation=name)
        with pipe.launch_log() as log:
            outs.append(pipe.apply_device(frames, "mono8" if cn == 1 else "bgr8").cpu().numpy())
        assert [r["name"] for r in records(log)] == [AC.kernel_name(cn, "mean2")], log.text
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], A.resize_stack(trusted(*src, 2, cn), dst[1], dst[0]))


@pytest.mark.parametrize("cn", (1, 3))
def test_ties_of_whole_factor_block_sums_round_half_to_even(rip_lib, oracle, cn):
    frames = trusted_of(("ties", cn))
    log = run_case(cn, (24, 8), (6, 2), "native%d" % cn, frames=frames)
    assert_one_launch(log, cn, (24, 8), (6, 2), 1)
    assert A.resize(AC.tie_frame(1), 2, 6).tolist() == [[0, 2, 2, 4, 4, 6], [0, 1, 1, 2, 252, 252]]   # what the frame was crafted for


@pytest.mark.parametrize("cn", (1, 3))
def test_flat_255_frames_stay_255(rip_lib, oracle, cn):
    for name, src, dst in (("flat512", (512, 256), (2, 1)), ("flat153", (153, 128), (40, 30))):
        frames = trusted_of((name, cn))
        run_case(cn, src, dst, "native%d" % cn, frames=frames)
        assert (A.resize(frames[0], dst[1], dst[0]) == 255).all()


def test_source_spans_start_at_every_byte_alignment_of_a_dword():
    """Three channels: the first byte of an output column's span is 3 * xfirst; the shapes above cover all four alignments, for the
    tap lists and for the block sums."""
    assert {int(3 * f) % 4 for f in A.tables(10, 41, 9, 40)["xfirst"]} == {0, 1, 2, 3}
    assert {(3 * 3 * x) % 4 for x in range(67)} == {0, 1, 2, 3}


# ---- destinations and formats ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", (1, 2, 3))
@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("fmt", ("native3", "native1"))
def test_pitched_and_offset_destinations(rip_lib, oracle, fmt, pitch, offset):
    """Row padding, the gaps between frames and the bytes around the batch keep their sentinels, with the base 1, 2 and 3 bytes off."""
    cn = 1 if fmt == "native1" else 3
    run_case(cn, (98, 14), (65, 9), fmt, n=3, pitch=pitch, gap=True, offset=offset, seed=4)       # tap lists
    run_case(cn, (195, 24), (65, 8), fmt, n=3, pitch=pitch, gap=True, offset=offset, seed=4)      # block sums


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("fmt", ("rgb8", "mono8", "rgb_chw_f16", "bgr_chw_f32"))
def test_pitched_destinations_under_a_format(rip_lib, oracle, fmt, pitch):
    run_case(3, (98, 14), (65, 9), fmt, n=3, pitch=pitch, gap=True, offset=1, seed=4)
    run_case(3, (195, 24), (65, 8), fmt, n=3, pitch=pitch, seed=4)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_every_format_behind_the_area_resize(rip_lib, oracle, fmt):
    """The converter runs unchanged on F': exactly one area launch in front of exactly one converter launch."""
    for src, dst in (((200, 29), (133, 19)), ((201, 27), (67, 9)), ((266, 38), (133, 19))):
        log = run_case(3, src, dst, fmt, n=3)
        names = [n for n in log.names() if n.startswith(KERNELS)]
        assert names == [AC.kernel_name(3, AC.kind_of(src, dst)), OV.KERNEL_OF_FORMAT[fmt]], log.text
        assert log.names()[-2:] == names


def test_mono8_on_a_one_channel_result_stays_the_identity_on_the_resized_image(rip_lib, oracle):
    log = run_case(1, (200, 29), (133, 19), "mono8")
    assert [r["name"] for r in records(log)] == [AV.kernel_name(1, False)] and "output_convert" not in log.text


@pytest.mark.parametrize("case", AV.CASES, ids=AV.case_id)
def test_every_variant_of_the_companion_runs_and_equals_the_reference(rip_lib, oracle, case):
    import torch
    (sw, sh), (dw, dh) = case.src_size, case.dst_size
    frames, e = noise(sw, sh, case.n_frames, case.channels, seed=5), trusted(sw, sh, case.n_frames, case.channels, 5)
    pipe = area_pipe((dw, dh))
    with pipe.launch_log() as log:
        out = pipe.apply_device(torch.from_numpy(frames.copy()).cuda(), case.encoding)
        torch.cuda.synchronize()
    assert (case.name, case.fc) in log.keys() and sum(n.startswith(KERNELS[:2]) for n in log.names()) == 1, log.text
    assert np.array_equal(out.cpu().numpy(), A.resize_stack(e, dh, dw))


# ---- batches, and switching the filter on one handle -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 3, 17))
def test_resident_batches(rip_lib, oracle, n):
    import torch
    src, dst = (153, 128), (40, 30)
    pipe = area_pipe(dst)
    out = pipe.apply_device(torch.from_numpy(noise(*src, n, 3, seed=6).copy()).cuda(), "bgr8")
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), A.resize_stack(trusted(*src, n, 3, 6), dst[1], dst[0]))


def test_switching_linear_and_area_on_one_handle_at_fixed_sizes(rip_lib, oracle):
    """The handle keeps one set of tables: the same four sizes under the other filter must not find the wrong set."""
    import torch
    src, dst = (98, 14), (65, 9)
    frames = torch.from_numpy(noise(*src, 2, 3, seed=7).copy()).cuda()
    e = trusted(*src, 2, 3, 7)
    linear = np.stack([oracle.resize_linear(np.ascontiguousarray(f), dst[1], dst[0]) for f in e])
    area = A.resize_stack(e, dst[1], dst[0])
    assert not np.array_equal(linear, area)
    pipe = area_pipe(dst, interpolation="linear")
    for name in ("linear", "area", "area", "linear", "linear", "area"):
        pipe.set_output_interpolation(name)
        with pipe.launch_log() as log:
            out = pipe.apply_device(frames, "bgr8").cpu().numpy()
        assert np.array_equal(out, area if name == "area" else linear), name
        assert [r["name"] for r in records(log)] == ["area_reduce_kernel<3, false>" if name == "area" else "resize_kernel<3, false>"], log.text
    pipe.set_output_size(*src)                         # F's own size under area: no launch, F itself
    with pipe.launch_log() as log:
        out = pipe.apply_device(frames, "bgr8").cpu().numpy()
    assert np.array_equal(out, e) and not records(log)
    pipe.set_output_size(0, 0)                         # the setting alone has no effect
    with pipe.launch_log() as log:
        out = pipe.apply_device(frames, "bgr8").cpu().numpy()
    assert np.array_equal(out, e) and not records(log)


# ---- the area resize behind the real pipeline ----------------------------------------------------------------------------------------
AFTER_FORMATS = ("native", "rgb_chw_f16", "mono8")


def run_behind(pipe, batch, enc, expectations, what, **kw):
    """The batch under every format of AFTER_FORMATS on one handle, each with another kind of target (tap lists, block sums, the
    2 x 2 mean), then with F's own size; expectations: E per frame."""
    import torch
    e = np.stack(expectations)
    rows, cols = e.shape[1:3]
    assert cols % 2 == 0 and rows % 4 == 0
    targets = ((cols * 10 // 17, rows * 10 // 17), (cols // 2, rows // 4), (cols // 2, rows // 2))
    pipe.set_output_interpolation("area")
    for fmt, (w, h) in zip(AFTER_FORMATS, targets):
        pipe.set_output_format(fmt)
        pipe.set_output_normalization(*NORM)
        pipe.set_output_size(w, h)
        with pipe.launch_log() as log:
            out = pipe.apply_device(batch, enc, **kw)
            torch.cuda.synchronize()
        ref = want(e, h, w, fmt)
        assert tuple(out.shape) == ref.shape, (what, fmt, out.shape, ref.shape)
        got = delivered(out)
        assert np.array_equal(got, R.bits(ref)), "%s %s -> %dx%d: %d of %d elements differ" % (what, fmt, w, h, int((got != R.bits(ref)).sum()), got.size)
        tail = [n for n in log.names() if n.startswith(KERNELS)]
        assert tail == [AC.kernel_name(3, AC.kind_of((cols, rows), (w, h)))] + ([OV.KERNEL_OF_FORMAT[fmt]] if fmt != "native" else []), log.text
        assert log.names()[-len(tail):] == tail, log.text
    pipe.set_output_format("native")
    pipe.set_output_size(cols, rows)
    with pipe.launch_log() as log:
        out = pipe.apply_device(batch, enc, **kw)
        torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), e), what
    assert not [n for n in log.names() if n.startswith(KERNELS)], log.text


def test_after_the_full_chain_with_undistortion_and_a_new_image_size(rip_lib, oracle):
    import torch
    import resize_reference as Z
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
    run_behind(pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_grbg8", refs, "full chain + undistortion")
    rows, cols = refs[0].shape[:2]                     # the camera matrix of the delivered image: the linear formula
    pipe.set_output_size(64, 40)
    hh, ww, k, pr = pipe.get_output_camera_info(h, w, 1, "bayer_grbg8")
    wk, wp = Z.scaled_camera(pipe.get_rect_camera_matrix(), pipe.get_rect_projection_matrix(), rows, cols, 40, 64)
    assert (hh, ww) == (40, 64) and np.array_equal(k, wk) and np.array_equal(pr, wp)


def test_after_the_chain_under_both_contraction_models(rip_lib, oracle):
    """The chain's bytes differ between the models; the area resize of the same F is the same under both (rip_set_fp_contraction does
    not reach it): the uncontracted frames go through handles of both models by way of a bgr8 input with every stage off."""
    import torch
    w, h = V.CHAIN_SIZE
    c = cfg(ce=True, ce_hue=1.3, ce_sat=0.7, ce_val=1.1, **FULL)
    frames = bayer_frames(w, h, "rggb")
    for fc in (0, 1):
        pipe = RawImagePipeline(False, "", "", "", device=0)
        configure(pipe, c)
        pipe.set_fp_contraction(fc)
        with oracle.fp_contraction(fc):
            refs = [oracle_run(oracle, c, f, "bayer_rggb8")[0] for f in frames]
        run_behind(pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_rggb8", refs, "chain fc=%d" % fc)
    outs = []
    for fc in (0, 1):
        pipe = area_pipe((80, 42))
        pipe.set_fp_contraction(fc)
        outs.append(pipe.apply_device(torch.from_numpy(np.stack(refs)).cuda(), "bgr8").cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], A.resize_stack(np.stack(refs), 42, 80))


def test_after_flip_90(rip_lib, oracle):
    import torch
    w, h = V.CHAIN_SIZE
    c = cfg(flip=True, flip_angle=90, **FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    frames = bayer_frames(w, h, "gbrg")
    refs = [oracle_run(oracle, c, f, "bayer_gbrg8")[0] for f in frames]
    assert refs[0].shape == (w, h, 3)
    run_behind(pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_gbrg8", refs, "flip 90")


def test_after_mht(rip_lib, oracle):
    import torch
    w, h = V.CHAIN_SIZE
    c = cfg(**FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_debayer_method("mht")
    frames = bayer_frames(w, h, "bggr")
    refs = [expected_mht(oracle, c, f, "bayer_bggr8")[0] for f in frames]
    run_behind(pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_bggr8", refs, "mht")


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
    run_behind(pipe, torch.from_numpy(batch).cuda(), G.enc16("rggb"), refs, "raw16")
    pipe.set_debayer_16bit_range(256, 4095)
    samples = [(f.astype(np.uint32) * 4).clip(0, 4095).astype(np.uint16) for f in frames]
    refs = [expected_raw16(oracle, c, f, "rggb", "bilinear", 256, 4095)[0] for f in samples]
    packed = np.stack([PKR.pack(f, "12p") for f in samples])
    run_behind(pipe, torch.from_numpy(packed).cuda(), PKR.enc("rggb", "12p"), refs, "packed 12p", width=w)


def ccc_pipe(c, filt, bias):
    p = RawImagePipeline(False, "", "", "", device=0)
    p.set_ccc_model(filt, bias)
    p.set_ccc_kalman_model(1.0, 10.0)
    configure(p, c)
    p.reset_white_balance_temporal_consistency()
    return p


def test_ccc_sequence_keeps_its_track_against_a_native_size_twin(rip_lib, oracle):
    """Five frames with temporal consistency on a handle with an area target and on a twin without a target: the same track and
    gains (the stage is downstream), the same taps; the delivered frame is the area resize of the twin's."""
    w, h, n = V.CHAIN_SIZE[0], V.CHAIN_SIZE[1], 5
    tw, th = w * 10 // 17, h * 10 // 17
    filt, bias = synth.ccc_model()
    c = cfg(wb=True, wb_method="ccc", wb_bright=0.8, wb_dark=0.2, wb_temporal=True, gamma=True, gamma_k=0.9)
    pipes = [ccc_pipe(c, filt, bias), ccc_pipe(c, filt, bias)]
    pipes[0].set_output_interpolation("area")
    pipes[0].set_output_size(tw, th)
    occ = oracle.CCC(filt, bias)
    occ.set_kalman_model(1.0, 10.0)
    for i in range(n):
        frame = synth.gen_frame(w, h, "bayer_gbrg8", seed=4100 + i, kind="scene", tint=(0.70 + 0.04 * i, 1.0, 0.55))
        ref = oracle_run(oracle, c, frame, "bayer_gbrg8", ccc=occ)[0]
        got, twin = (p.process(frame, "bayer_gbrg8") for p in pipes)
        assert np.array_equal(twin, ref), "twin without a target, frame %d" % i
        assert got.shape == (th, tw, 3) and np.array_equal(got, A.resize(ref, th, tw)), "frame %d" % i
        assert np.array_equal(pipes[0].get_ccc_track(1), pipes[1].get_ccc_track(1))
        assert np.array_equal(pipes[0].get_white_balance_info(1), pipes[1].get_white_balance_info(1))
        for getter in ("get_dist_debayered_image", "get_dist_color_image"):
            a, b = getattr(pipes[0], getter)(), getattr(pipes[1], getter)()
            assert a.shape == (h, w, 3) and np.array_equal(a, b), getter
        assert pipes[0].get_processed_image().size == 0 and np.array_equal(pipes[1].get_processed_image(), ref)


# ---- host paths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ("native", "rgb8", "rgb_chw_f16"))
def test_host_paths(rip_lib, oracle, fmt):
    w, h, tw, th = 74, 58, 21, 17
    c = cfg(**FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_output_format(fmt)
    pipe.set_output_normalization(*NORM)
    pipe.set_output_interpolation("area")
    pipe.set_output_size(tw, th)
    frames = bayer_frames(w, h, "rggb", 3)
    refs = [oracle_run(oracle, c, f, "bayer_rggb8")[0] for f in frames]
    wants = [want(e[None], th, tw, fmt)[0] for e in refs]
    enc = "bgr8" if fmt == "native" else fmt

    def same(got, k, what):
        assert got.shape == wants[k].shape and got.dtype == wants[k].dtype, (what, got.shape, got.dtype)
        assert np.array_equal(R.bits(got), R.bits(wants[k])), "%s %s" % (fmt, what)
    same(pipe.process(frames[0], "bayer_rggb8"), 0, "process")
    assert pipe.last_encoding == enc and pipe.get_processed_image().size == 0
    t = [pipe.submit(f, "bayer_rggb8") for f in frames[:2]]
    same(pipe.collect(t[0]), 0, "collect copy")
    same(pipe.collect(t[1], copy=False), 1, "collect view")
    pinned = P.host_alloc(wants[2].shape, wants[2].dtype)
    pinned.view(np.uint8)[...] = SENTINEL
    assert pipe.collect(pipe.submit(frames[2], "bayer_rggb8", out=pinned)) is pinned
    same(pinned, 2, "submit into a pinned array")
    pipe.set_output_size(37, 29)                       # another target between frames (whole 2 x 2 is the mean), then linear again
    got = pipe.process(frames[1], "bayer_rggb8")
    assert np.array_equal(R.bits(got), R.bits(want(refs[1][None], 29, 37, fmt)[0]))
    pipe.set_output_interpolation("linear")
    pipe.set_output_size(tw, th)
    got = pipe.process(frames[2], "bayer_rggb8")
    lin = oracle.resize_linear(refs[2], th, tw)
    assert np.array_equal(R.bits(got), R.bits(lin if fmt == "native" else R.convert(lin[None], fmt, *NORM)[0]))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing_and_leave_the_ccc_state_alone(rip_lib, oracle):
    """An enlarging target and a factor above 256 under "area" fail the frame call before anything is enqueued: the ccc filter of the
    handle has not moved, so the next frames equal the oracle's sequence."""
    import torch
    w, h = V.CHAIN_SIZE
    tw, th = w * 10 // 17, h * 10 // 17
    filt, bias = synth.ccc_model()
    c = cfg(wb=True, wb_method="ccc", wb_bright=0.8, wb_dark=0.2, wb_temporal=True)
    pipe = ccc_pipe(c, filt, bias)
    pipe.set_output_interpolation("area")
    pipe.set_output_size(tw, th)
    occ = oracle.CCC(filt, bias)
    occ.set_kalman_model(1.0, 10.0)
    frames = [synth.gen_frame(w, h, "bayer_rggb8", seed=900 + i, tint=(0.6 + 0.1 * i, 1.0, 0.5)) for i in range(3)]

    def expect(f):
        return A.resize(oracle_run(oracle, c, f, "bayer_rggb8", ccc=occ)[0], th, tw)
    assert np.array_equal(pipe.process(frames[0], "bayer_rggb8"), expect(frames[0]))
    batch = torch.from_numpy(np.stack(frames)).cuda()
    tall = np.zeros((514, 8), np.uint8)
    with pipe.launch_log() as log:
        for target in ((w + 1, h), (w, h + 1), (2 * w, 2 * h)):                           # (a)
            pipe.set_output_size(*target)
            for call in (lambda: pipe.process(frames[1], "bayer_rggb8"), lambda: pipe.submit(frames[1], "bayer_rggb8"),
                         lambda: pipe.apply_device(batch, "bayer_rggb8"), lambda: pipe.query_output(h, w, 1, "bayer_rggb8")):
                with pytest.raises(ValueError) as e:
                    call()
                assert "downscale" in str(e.value)
        pipe.set_output_size(8, 2)                                                          # (b): 514 rows to 2
        for call in (lambda: pipe.process(tall, "bayer_rggb8"), lambda: pipe.submit(tall, "bayer_rggb8")):
            with pytest.raises(ValueError) as e:
                call()
            assert "256" in str(e.value)
        torch.cuda.synchronize()
    assert not log.records(), log.text
    pipe.set_output_size(tw, th)
    for f in frames[1:]:
        assert np.array_equal(pipe.process(f, "bayer_rggb8"), expect(f))


# ---- a seeded fuzz ----------------------------------------------------------------------------------------------------------------
FUZZ_FORMATS = ("native",) + R.FORMATS


@pytest.mark.parametrize("seed", range(AC.FUZZ_CASES))
def test_fuzz(rip_lib, oracle, seed):
    k = AC.fuzz_case(seed)
    cn = k["cn"]
    fmt = FUZZ_FORMATS[k["fmt"] % len(FUZZ_FORMATS)] if cn == 3 else ("native", "mono8")[k["fmt"] % 2]
    fmt = "native%d" % cn if fmt == "native" else fmt
    log = run_case(cn, k["src"], k["dst"], fmt, n=k["n"], pitch=PITCHES[k["pitch"]], gap=k["gap"], offset=int(k["base_off"]) * (1 + seed % 3),
                   seed=100 + seed)
    kind = AC.kind_of(k["src"], k["dst"])
    expect = [] if kind == "identity" else [AC.kernel_name(cn, kind)]                       # a target of F's own size launches nothing
    assert [r["name"] for r in records(log)] == expect, (k, log.text)
