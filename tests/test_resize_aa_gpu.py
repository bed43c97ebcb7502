"""The resize stage under "linear_aa" and "cubic_aa" on the GPU (include/rip.h rip_set_output_interpolation): what the frame calls
deliver equals, byte for byte (float formats as bit patterns), tests/aa_reference.py -- which tests/test_resize_aa.py pins to
torch.nn.functional.interpolate(uint8, antialias=True) -- applied to the image E the suite already trusts for that input
(helpers.oracle_run), and not one byte outside the delivered elements is written.  Tolerance 0 everywhere.

Sizes come from the launch code (rip_aa.hpp: a workgroup owns 64 output columns x TH output rows, TH the largest of 8, 4, 2, 1 whose
source rows fit 64 KiB of LDS): tests/aa_cases.py lists target widths 63 / 64 / 65 / 129 and heights 7 / 8 / 9 / 17, upscales,
skipped passes, one-pixel sides and a tall narrow frame per tile height.  Sources stay below about 300 x 300 apart from those."""
import functools

import numpy as np
import pytest

import aa_cases as AC
import aa_reference as A
import aa_variant_cases as AV
import fit_reference as FR
import output_reference as R
import output_variant_cases as OV
import variant_cases as V
from helpers import cfg, configure, device_batch, oracle_params, oracle_run
from raw_image_pipeline_amd import RawImagePipeline, synth
from raw_image_pipeline_amd import pipeline as P
from test_output_format_gpu import FULL, NORM, PITCHES, SENTINEL, bayer_frames, delivered
from test_resize_area_gpu import ccc_pipe, destination
from test_resize_gpu import LAYOUT_OF, apply_into, noise, trusted

pytestmark = pytest.mark.gpu

RESIZE_KERNELS = ("aa_kernel", "area_reduce_kernel", "resize_kernel", "fit_")
KERNELS = RESIZE_KERNELS + ("output_convert",)
NAMES = AC.FILTER_NAMES


def expected(F, name, roi=None, target=None, fit="stretch", pad=FR.PAD_DEFAULT):
    """PARITY.md "Resize: window and fit" with the picture's bytes from aa_reference: the window alone decides them."""
    F = np.asarray(F)
    (x, y, w, h), (left, top, wi, hi), (W, H) = FR.geometry(F.shape[1], F.shape[0], roi, target, fit)
    channels = 1 if F.ndim == 2 else 3
    canvas = np.empty((H, W) + F.shape[2:], np.uint8)
    canvas[...] = np.array(FR.pad_bytes(pad, channels), np.uint8) if channels == 3 else FR.pad_bytes(pad, 1)[0]
    window = np.ascontiguousarray(F[y:y + h, x:x + w])
    canvas[top:top + hi, left:left + wi] = window if (h, w) == (hi, wi) else A.resize(window, hi, wi, name)
    return canvas


def want(e, name, fmt, **geom):
    """What a handle under filter `name` and format fmt delivers for the trusted frames e."""
    r = np.stack([expected(f, name, **geom) for f in e])
    if fmt in ("native", "native1", "native3") or (fmt == "mono8" and r.ndim == 3):
        return r
    return R.convert(r, fmt, *NORM)


def aa_pipe(name, target, fmt="native", roi=None, fit="stretch"):
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, cfg())
    pipe.set_output_format(fmt)
    pipe.set_output_normalization(*NORM)
    pipe.set_output_interpolation(name)
    if roi is not None:
        pipe.set_output_roi(*roi)
    pipe.set_output_fit(fit)
    if target is not None:
        pipe.set_output_size(*target)
    return pipe


def records(log):
    return [r for r in log.records() if r["name"].startswith(RESIZE_KERNELS)]


def run_case(name, cn, src, dst, fmt, n=2, pitch="tight", gap=False, offset=0, seed=0, frames=None, roi=None, fit="stretch", pipe=None):
    """Frames of src = (w, h) -- noise unless given -- under filter `name`, window roi and fit mode, resized to dst = (w, h) under fmt
    into a sentinel-filled destination."""
    import torch
    (sw, sh), (dw, dh) = src, dst
    if frames is None:
        frames, e = noise(sw, sh, n, cn, seed), trusted(sw, sh, n, cn, seed)
    else:
        e, n = frames, len(frames)
    pipe = pipe or aa_pipe(name, (dw, dh), "native" if fmt.startswith("native") else fmt, roi, fit)
    d = destination(LAYOUT_OF.get(fmt, fmt), n, dh, dw, pitch=pitch, gap=gap, offset=offset)
    with pipe.launch_log() as log:
        apply_into(pipe, torch.from_numpy(np.array(frames)).cuda(), "mono8" if cn == 1 else "bgr8", d.view)
    d.check(want(e, name, fmt, roi=roi, target=dst, fit=fit), "%s %s %dx%dx%d roi %s %s -> %dx%d %s offset %d" % (name, fmt, sw, sh, cn, roi, fit, dw, dh, pitch, offset))
    return log


def assert_one_aa_launch(log, name, cn, window_wh, picture_wh, n, windowed=False, padded=False):
    """The launch log names aa_kernel<...> and no other resize kernel (the letterbox adds its pad launch); the grid is the tile
    height the reference derives."""
    rec = records(log)
    assert [r["name"] for r in rec] == [AC.kernel_name(cn, windowed)] + (["fit_pad_kernel<%d>" % cn] if padded else []), log.text
    th = A.tile_rows(name, window_wh[1], picture_wh[1], cn)[0]
    grid = ((picture_wh[0] + AC.TILE_W - 1) // AC.TILE_W, (picture_wh[1] + th - 1) // th)
    assert rec[0]["grid"] == grid and rec[0]["block"] == 256 and rec[0]["frames"] == n and rec[0]["fc"] == 0, (rec, th)
    return th


# ---- the kernel's indexing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", (1, 3))
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", AC.SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s.src + s.dst))
def test_tile_edges_upscales_skipped_passes_and_one_pixel_sides(rip_lib, oracle, shape, name, cn):
    log = run_case(name, cn, shape.src, shape.dst, "native%d" % cn)
    assert_one_aa_launch(log, name, cn, shape.src, shape.dst, 2)
    assert "output_convert" not in log.text


def test_every_tile_height_the_host_chooses_runs(rip_lib, oracle):
    """A tall narrow frame per tile height.  Under the factor cap the host never has to go below 2 (two cubic output rows at a factor
    of 64 read 321 source rows: 61 632 bytes with three channels); a height of 1 runs in the host-run test of tests/test_resize_aa.py."""
    seen = set()
    for name, cn, src, dst in AC.TILE_HEIGHT_SHAPES:
        log = run_case(name, cn, src, dst, "native%d" % cn, n=1, seed=3)
        seen.add(assert_one_aa_launch(log, name, cn, src, dst, 1))
    assert seen == {8, 4, 2}


@pytest.mark.parametrize("cn", (1, 3))
def test_clamping_on_both_sides_under_the_cubic_filter(rip_lib, oracle, cn):
    for src, dst in (((120, 90), (70, 41)), ((40, 30), (90, 70))):
        frames = AC.binary_noise(*src, 2, cn, seed=1)
        e = np.stack([oracle_run(oracle, cfg(), np.ascontiguousarray(f), "mono8" if cn == 1 else "bgr8")[0].reshape(f.shape) for f in frames])
        assert np.array_equal(e, frames)                 # every stage off: F is the input
        unclipped = []
        A.resize(frames[0], dst[1], dst[0], "cubic_aa", unclipped)
        assert len(unclipped) == 2 and all(lo < 0 and hi > 255 for lo, hi in unclipped), unclipped     # both passes leave [0, 255] on both sides
        run_case("cubic_aa", cn, src, dst, "native%d" % cn, frames=frames)


# ---- windows and fit modes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", (1, 3))
@pytest.mark.parametrize("x", (0, 1, 2, 3))
def test_window_origins_at_every_byte_phase(rip_lib, oracle, x, cn):
    """Column x of a row that starts 16-byte aligned: byte phase x (one channel) or 3 x mod 4 (three) of the window's first tap; the
    window ends at F's last column for x = 3, where the last dword of the row is the last one that may be read."""
    src = (83, 41)
    roi = (x, 1 + x, 80, 37)
    for name, dst in (("linear_aa", (33, 15)), ("cubic_aa", (65, 9)), ("cubic_aa", (100, 50)), ("linear_aa", (80, 20))):
        log = run_case(name, cn, src, dst, "native%d" % cn, roi=roi, seed=x)
        assert_one_aa_launch(log, name, cn, roi[2:], dst, 2, windowed=True)
    assert {(3 * v) % 4 for v in (0, 1, 2, 3)} == {0, 1, 2, 3}


@pytest.mark.parametrize("cn", (1, 3))
@pytest.mark.parametrize("name", NAMES)
def test_crop_and_letterbox_with_bands(rip_lib, oracle, name, cn):
    src = (150, 60)
    for fit, roi, dst in (("crop", None, (40, 40)), ("crop", (7, 3, 100, 50), (30, 45)), ("letterbox", None, (70, 70)), ("letterbox", (5, 2, 90, 57), (64, 80)),
                          ("letterbox", None, (301, 130))):
        log = run_case(name, cn, src, dst, "native%d" % cn, roi=roi, fit=fit, pitch="pitch16", gap=True, offset=1)
        (x, y, w, h), (left, top, wi, hi), _ = FR.geometry(src[0], src[1], roi, dst, fit)
        assert_one_aa_launch(log, name, cn, (w, h), (wi, hi), 2, windowed=(x, y, w, h) != (0, 0) + src, padded=(wi, hi) != dst)
    assert FR.geometry(150, 60, None, (70, 70), "letterbox")[1][2:] != (70, 70)       # there are bands


def test_a_window_of_the_pictures_size_stays_the_copy(rip_lib, oracle):
    log = run_case("cubic_aa", 3, (90, 50), (40, 30), "native3", roi=(11, 7, 40, 30))
    assert [r["name"] for r in records(log)] == ["fit_linear_kernel<3>"], log.text


# ---- destinations and formats ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", (1, 2, 3))
@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("fmt", ("native3", "native1"))
def test_pitched_and_offset_destinations(rip_lib, oracle, fmt, pitch, offset):
    """Row padding, the gaps between frames and the bytes around the batch keep their sentinels, with the base 1, 2 and 3 bytes off."""
    cn = 1 if fmt == "native1" else 3
    run_case(NAMES[offset % 2], cn, (150, 111), (65, 9), fmt, n=3, pitch=pitch, gap=True, offset=offset, seed=4)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_every_format_behind_the_filter(rip_lib, oracle, fmt):
    """The converter runs unchanged on F': exactly one aa launch in front of exactly one converter launch."""
    for k, (src, dst) in enumerate((((200, 29), (133, 19)), ((37, 29), (80, 61)))):
        name = NAMES[(k + len(fmt)) % 2]
        log = run_case(name, 3, src, dst, fmt, n=3, pitch=PITCHES[k], offset=k)
        names = [n for n in log.names() if n.startswith(KERNELS)]
        assert names == [AC.kernel_name(3, False), OV.KERNEL_OF_FORMAT[fmt]], log.text
        assert log.names()[-2:] == names


def test_mono8_on_a_one_channel_result_stays_the_identity_on_the_resized_image(rip_lib, oracle):
    log = run_case("linear_aa", 1, (200, 29), (133, 19), "mono8")
    assert [r["name"] for r in records(log)] == [AC.kernel_name(1, False)] and "output_convert" not in log.text


@pytest.mark.parametrize("case", AV.CASES, ids=AV.case_id)
def test_every_variant_of_the_companion_runs_and_equals_the_reference(rip_lib, oracle, case):
    import torch
    (sw, sh), (dw, dh) = case.frame_size, case.dst_size
    frames, e = noise(sw, sh, case.n_frames, case.channels, seed=5), trusted(sw, sh, case.n_frames, case.channels, 5)
    pipe = aa_pipe(case.filter, (dw, dh), roi=case.roi)
    with pipe.launch_log() as log:
        out = pipe.apply_device(torch.from_numpy(frames.copy()).cuda(), case.encoding)
        torch.cuda.synchronize()
    assert (case.name, case.fc) in log.keys() and sum(n.startswith(RESIZE_KERNELS) for n in log.names()) == 1, log.text
    assert np.array_equal(out.cpu().numpy(), want(e, case.filter, "native", roi=case.roi, target=case.dst_size))


# ---- behind the real pipeline -----------------------------------------------------------------------------------------------------
def test_after_the_full_chain_with_undistortion(rip_lib, oracle):
    import torch
    import resize_reference as Z
    w, h = V.REMAP_SIZE
    cam = synth.camera_model(w, h)
    c = cfg(cam=cam, undistort=True, flip=True, flip_angle=180, **FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    newK = oracle.fisheye_new_camera_matrix(cam["K"], cam["D"], (w, h), cam["R"], c["balance"], None, c["fov_scale"])
    mx, my = oracle.fisheye_maps(cam["K"], cam["D"], cam["R"], newK, (w, h))
    frames = bayer_frames(w, h, "grbg")
    refs = []
    for f in frames:
        keep = []
        prm = oracle_params(oracle, c, keep)
        prm.map_x, prm.map_y = mx.ctypes.data, my.ctypes.data
        prm.map_rows, prm.map_cols = mx.shape
        refs.append(oracle.pipeline(prm, f, "bayer_grbg8")[0])
    e = np.stack(refs)
    rows, cols = e.shape[1:3]
    batch = torch.from_numpy(np.stack(frames)).cuda()
    for name, fmt, (tw, th) in (("cubic_aa", "rgb_chw_f16", (cols * 10 // 23, rows * 10 // 23)), ("linear_aa", "native", (cols * 3 // 2, rows // 3))):
        pipe.set_output_interpolation(name)
        pipe.set_output_format(fmt)
        pipe.set_output_normalization(*NORM)
        pipe.set_output_size(tw, th)
        with pipe.launch_log() as log:
            out = pipe.apply_device(batch, "bayer_grbg8")
            torch.cuda.synchronize()
        ref = want(e, name, fmt, target=(tw, th))
        assert tuple(out.shape) == ref.shape, (name, fmt, out.shape, ref.shape)
        assert np.array_equal(delivered(out), R.bits(ref)), (name, fmt)
        tail = [n for n in log.names() if n.startswith(KERNELS)]
        assert tail == [AC.kernel_name(3, False)] + ([OV.KERNEL_OF_FORMAT[fmt]] if fmt != "native" else []), log.text
        assert log.names()[-len(tail):] == tail, log.text
    pipe.set_output_size(64, 40)                       # the camera matrix of the delivered image: the linear formula
    hh, ww, k, pr = pipe.get_output_camera_info(h, w, 1, "bayer_grbg8")
    wk, wp = Z.scaled_camera(pipe.get_rect_camera_matrix(), pipe.get_rect_projection_matrix(), rows, cols, 40, 64)
    assert (hh, ww) == (40, 64) and np.array_equal(k, wk) and np.array_equal(pr, wp)


def test_the_result_does_not_depend_on_the_contraction_model(rip_lib, oracle):
    import torch
    e = trusted(98, 57, 2, 3, 8)
    outs = []
    for fc in (0, 1):
        pipe = aa_pipe("cubic_aa", (41, 23))
        pipe.set_fp_contraction(fc)
        outs.append(pipe.apply_device(torch.from_numpy(noise(98, 57, 2, 3, 8).copy()).cuda(), "bgr8").cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], A.resize_stack(e, 23, 41, "cubic_aa"))


# ---- handle state ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ("pitch16", "base_off", "frame_gap"))
def test_a_resident_batch_of_five_frames_in_a_strided_layout(rip_lib, oracle, layout):
    import torch
    src, dst, n = (153, 128), (40, 30), 5
    b = device_batch(noise(*src, n, 3, seed=6), layout, np.random.default_rng(1))
    pipe = aa_pipe("linear_aa", dst)
    out = pipe.apply_device(b.view, "bgr8")
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), A.resize_stack(trusted(*src, n, 3, 6), dst[1], dst[0], "linear_aa"))
    b.check_padding(layout)


def test_switching_among_the_four_filters_on_one_handle_at_fixed_sizes(rip_lib, oracle):
    """The handle keeps one set of tables: the same four sizes under another filter must not find the wrong set."""
    import torch
    import area_reference as AR
    src, dst = (98, 14), (65, 9)
    frames = torch.from_numpy(noise(*src, 2, 3, seed=7).copy()).cuda()
    e = trusted(*src, 2, 3, 7)
    outs = {"linear": np.stack([oracle.resize_linear(np.ascontiguousarray(f), dst[1], dst[0]) for f in e]), "area": AR.resize_stack(e, dst[1], dst[0]),
            "linear_aa": A.resize_stack(e, dst[1], dst[0], "linear_aa"), "cubic_aa": A.resize_stack(e, dst[1], dst[0], "cubic_aa")}
    kernel = {"linear": "resize_kernel<3, false>", "area": "area_reduce_kernel<3, false>", "linear_aa": "aa_kernel<3, false>", "cubic_aa": "aa_kernel<3, false>"}
    assert len({v.tobytes() for v in outs.values()}) == 4
    pipe = aa_pipe("linear", dst)
    for name in ("linear_aa", "cubic_aa", "cubic_aa", "area", "linear_aa", "linear", "cubic_aa", "area", "linear", "linear_aa"):
        pipe.set_output_interpolation(name)
        with pipe.launch_log() as log:
            out = pipe.apply_device(frames, "bgr8").cpu().numpy()
        assert np.array_equal(out, outs[name]), name
        assert [r["name"] for r in records(log)] == [kernel[name]], log.text
    pipe.set_output_size(*src)                         # F's own size: no launch, F itself
    with pipe.launch_log() as log:
        out = pipe.apply_device(frames, "bgr8").cpu().numpy()
    assert np.array_equal(out, e) and not records(log)
    pipe.set_output_size(49, 7)                        # exactly half: no 2 x 2 mean under these names
    with pipe.launch_log() as log:
        out = pipe.apply_device(frames, "bgr8").cpu().numpy()
    assert np.array_equal(out, A.resize_stack(e, 7, 49, "linear_aa")) and [r["name"] for r in records(log)] == ["aa_kernel<3, false>"], log.text


def test_ccc_sequence_keeps_its_track_against_a_native_twin_across_a_refused_frame(rip_lib, oracle):
    """Frames with temporal consistency on a handle with an antialiased target and on a twin without one: the same track and gains
    (the stage is downstream).  In between the handle is asked for a factor of 65 and refuses before anything is enqueued: the
    filter has not moved, so the frames after it still equal the twin's."""
    w, h, n = V.CHAIN_SIZE[0], V.CHAIN_SIZE[1], 4
    tw, th = w * 10 // 17, h * 10 // 17
    filt, bias = synth.ccc_model()
    c = cfg(wb=True, wb_method="ccc", wb_bright=0.8, wb_dark=0.2, wb_temporal=True, gamma=True, gamma_k=0.9)
    pipes = [ccc_pipe(c, filt, bias), ccc_pipe(c, filt, bias)]
    pipes[0].set_output_interpolation("cubic_aa")
    pipes[0].set_output_size(tw, th)
    occ = oracle.CCC(filt, bias)
    occ.set_kalman_model(1.0, 10.0)
    tall = np.zeros((130, 8), np.uint8)
    for i in range(n):
        frame = synth.gen_frame(w, h, "bayer_gbrg8", seed=4100 + i, kind="scene", tint=(0.70 + 0.04 * i, 1.0, 0.55))
        ref = oracle_run(oracle, c, frame, "bayer_gbrg8", ccc=occ)[0]
        if i == 2:                                     # 130 rows to 2: a factor of 65
            pipes[0].set_output_size(8, 2)
            with pipes[0].launch_log() as log:
                for call in (lambda: pipes[0].process(tall, "bayer_gbrg8"), lambda: pipes[0].submit(tall, "bayer_gbrg8"),
                             lambda: pipes[0].query_output(130, 8, 1, "bayer_gbrg8")):
                    with pytest.raises(ValueError) as err:
                        call()
                    assert "64 per axis" in str(err.value)
            assert not log.records(), log.text
            pipes[0].set_output_size(tw, th)
        got, twin = (p.process(frame, "bayer_gbrg8") for p in pipes)
        assert np.array_equal(twin, ref), "twin without a target, frame %d" % i
        assert got.shape == (th, tw, 3) and np.array_equal(got, A.resize(ref, th, tw, "cubic_aa")), "frame %d" % i
        assert np.array_equal(pipes[0].get_ccc_track(1), pipes[1].get_ccc_track(1))
        assert np.array_equal(pipes[0].get_white_balance_info(1), pipes[1].get_white_balance_info(1))
        assert pipes[0].get_processed_image().size == 0 and np.array_equal(pipes[1].get_processed_image(), ref)


# ---- host paths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ("native", "rgb_chw_f16"))
def test_host_paths(rip_lib, oracle, fmt):
    w, h, tw, th = 74, 58, 21, 17
    c = cfg(**FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_output_format(fmt)
    pipe.set_output_normalization(*NORM)
    pipe.set_output_interpolation("cubic_aa")
    pipe.set_output_size(tw, th)
    frames = bayer_frames(w, h, "rggb", 3)
    refs = [oracle_run(oracle, c, f, "bayer_rggb8")[0] for f in frames]
    wants = [want(e[None], "cubic_aa", fmt, target=(tw, th))[0] for e in refs]

    def same(got, k, what):
        assert got.shape == wants[k].shape and got.dtype == wants[k].dtype, (what, got.shape, got.dtype)
        assert np.array_equal(R.bits(got), R.bits(wants[k])), "%s %s" % (fmt, what)
    same(pipe.process(frames[0], "bayer_rggb8"), 0, "process")
    assert pipe.last_encoding == ("bgr8" if fmt == "native" else fmt) and pipe.get_processed_image().size == 0
    t = [pipe.submit(f, "bayer_rggb8") for f in frames[:2]]
    same(pipe.collect(t[0]), 0, "collect copy")
    same(pipe.collect(t[1], copy=False), 1, "collect view")
    pinned = P.host_alloc(wants[2].shape, wants[2].dtype)
    pinned.view(np.uint8)[...] = SENTINEL
    assert pipe.collect(pipe.submit(frames[2], "bayer_rggb8", out=pinned)) is pinned
    same(pinned, 2, "submit into a pinned array")
    pipe.set_output_interpolation("linear_aa")         # another filter and an enlarging target between frames
    pipe.set_output_size(90, 29)
    got = pipe.process(frames[1], "bayer_rggb8")
    assert np.array_equal(R.bits(got), R.bits(want(refs[1][None], "linear_aa", fmt, target=(90, 29))[0]))


# ---- a seeded fuzz ----------------------------------------------------------------------------------------------------------------
FUZZ_FORMATS = ("native",) + R.FORMATS


@pytest.mark.parametrize("seed", range(AC.FUZZ_CASES))
def test_fuzz(rip_lib, oracle, seed):
    k = AC.fuzz_case(seed)
    cn = k["cn"]
    fmt = FUZZ_FORMATS[k["fmt"] % len(FUZZ_FORMATS)] if cn == 3 else ("native", "mono8")[k["fmt"] % 2]
    fmt = "native%d" % cn if fmt == "native" else fmt
    log = run_case(k["name"], cn, k["src"], k["dst"], fmt, n=k["n"], pitch=PITCHES[k["pitch"]], gap=k["gap"], offset=int(k["base_off"]) * (1 + seed % 3),
                   seed=100 + seed)
    assert [r["name"] for r in records(log)] == [AC.kernel_name(cn, False)], (k, log.text)
