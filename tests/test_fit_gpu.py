"""The window and the fit modes of the resize stage on the GPU (include/rip.h rip_set_output_roi, rip_set_output_fit,
rip_set_output_pad): what the frame calls deliver equals, byte for byte (float formats as bit patterns),
``output_reference.convert(fit_reference.expected(E, ...), format)`` where E is the image the suite already trusts for that input --
the input itself with every stage off, else the oracle's -- and not one byte outside the delivered elements is written.  Tolerance 0
everywhere.  The shapes are those of tests/fit_cases.py, which the kernels-on-the-host test of tests/test_fit.py runs as well."""
import ctypes as C

import numpy as np
import pytest

import fit_cases as FC
import fit_reference as FR
import fit_variant_cases as FV
import output_reference as R
import output_variant_cases as OV
import packed_reference as PKR
import raw16_cases as G
import variant_cases as V
from helpers import cfg, configure, expected_mht, oracle_run
from raw16_reference import expected_raw16
from raw_image_pipeline_amd import RawImagePipeline, synth
from raw_image_pipeline_amd import pipeline as P
from test_output_format_gpu import FULL, NORM, SENTINEL, Destination, bayer_frames, delivered
from test_resize_gpu import apply_into

pytestmark = pytest.mark.gpu

STAGE = ("fit_", "resize_kernel", "area_reduce_kernel")          # the kernels of the resize stage, in any library
LAYOUTS = (("tight", False, False), ("pitch16", True, True), ("pitch_elem", True, False))      # (pitch, gap, base_off) of Destination


def plain_pipe():
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, cfg())
    pipe.set_output_normalization(*NORM)
    return pipe


def setup(pipe, c, fmt="native"):
    pipe.set_output_format(fmt)
    pipe.set_output_roi(*(c.roi or (0, 0, 0, 0)))
    pipe.set_output_size(*(c.target or (0, 0)))
    pipe.set_output_fit(c.fit)
    pipe.set_output_interpolation(c.interpolation)
    pipe.set_output_pad(*c.pad)


def want(frames, c, fmt):
    r = FR.expected_stack(frames, c.roi, c.target, c.fit, c.interpolation, c.pad)
    if fmt == "native" or (fmt == "mono8" and r.ndim == 3):
        return r
    return R.convert(r, fmt, *NORM)


def stage_names(log):
    return [n for n in log.names() if n.startswith(STAGE)]


def expected_names(c):
    src, dst, _ = FC.geometry(c)
    if src == dst == (0, 0) + c.size:                                 # all of F delivered as it is: the identity launches nothing
        return []
    name, padded = FC.kernel_of(c)
    return [name] + (["fit_pad_kernel<%d>" % c.channels] if padded else [])


def run_case(pipe, c, fmt="native", layout=LAYOUTS[0], seed=0):
    """The case's noise frames (no stage is on: F is the input) through rip_apply_device into a sentinel-filled destination: every
    byte of the buffer is compared, and the resize stage's launches are exactly the ones the case's geometry asks for."""
    import torch
    frames = FC.frames(c, seed)
    (W, H) = FC.geometry(c)[2]
    setup(pipe, c, fmt)
    dfmt = fmt if fmt != "native" else ("mono8" if c.channels == 1 else "rgb8")
    d = Destination(dfmt, c.n, H, W, pitch=layout[0], gap=layout[1], base_off=layout[2])
    with pipe.launch_log() as log:
        apply_into(pipe, torch.from_numpy(frames).cuda(), "mono8" if c.channels == 1 else "bgr8", d.view)
    d.check(want(frames, c, fmt), "%s %s %s" % (FC.case_id(c), fmt, layout[0]))
    assert stage_names(log) == expected_names(c), (FC.case_id(c), log.text)
    return log


# ---- the kernels' indexing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", (1, 3))
@pytest.mark.parametrize("group", ("origin", "lane", "tile", "band"))
def test_every_shape_of_the_kernels(rip_lib, group, cn):
    """The window's origin against dword alignment through every path, picture widths around a lane and a workgroup, the area
    kernels' tile edges, and the letterbox bands (tests/fit_cases.py), each under one of three destination layouts."""
    pipe = plain_pipe()
    cases = [c for c in getattr(FC, group + "_cases")() if c.channels == cn]
    assert len(cases) >= 13
    for i, c in enumerate(cases):
        run_case(pipe, c._replace(n=2), layout=LAYOUTS[i % 3])


def test_the_shapes_cover_what_they_claim():
    origins = FC.origin_cases()
    for path in ("linear", "mean2", "whole", "taps", "copy"):
        for cn in (1, 3):
            mine = [c for c in origins if c.channels == cn and FR.rule(FC.geometry(c)[0][2:], FC.geometry(c)[1][2:], c.interpolation) == path]
            assert {(c.roi[0] * cn) % 4 for c in mine} == {0, 1, 2, 3}, (path, cn)                                   # every byte phase of the first tap
            assert any(c.roi[0] + c.roi[2] == c.size[0] and c.roi[1] + c.roi[3] == c.size[1] for c in mine)          # the window ends with F
            assert all(FC.kernel_of(c)[0].startswith("fit_") for c in mine)
    lefts = {FC.geometry(c)[1][0] for c in FC.band_cases() if c.fit == "letterbox"}
    assert {0, 1, 2, 3, 5} <= lefts
    pics = [FC.geometry(c)[1][2:] for c in FC.band_cases()]
    assert any(p[1] == 1 for p in pics) and any(p[0] == 1 for p in pics)                                               # one row, one column
    odd = [c for c in FC.band_cases() if c.fit == "letterbox" and (c.target[0] - FC.geometry(c)[1][2]) % 2 == 1]
    assert odd
    assert len({c.pad for c in FC.band_cases()}) == 3


@pytest.mark.parametrize("v", FV.CASES, ids=FV.case_id)
def test_every_variant_of_the_companion_runs_and_equals_the_reference(rip_lib, v):
    log = run_case(plain_pipe(), v.case, seed=5)
    assert (v.name, v.fc) in log.keys(), log.text
    rec = [r for r in log.records() if r["name"] == v.name]
    assert len(rec) == 1 and rec[0]["frames"] == v.case.n and rec[0]["block"] == 256, rec


def test_equal_aspects_launch_no_pad_kernel(rip_lib):
    pipe = plain_pipe()
    for cn in (1, 3):
        for c in (FC.case(cn, (40, 30), None, (20, 15), "letterbox"), FC.case(cn, (40, 30), None, (28, 21), "letterbox", "area"),
                  FC.case(cn, (43, 31), (2, 1, 40, 30), (20, 15), "letterbox"), FC.case(cn, (40, 30), None, (20, 15), "crop")):
            log = run_case(pipe, c)
            assert "fit_pad_kernel" not in log.text and len(stage_names(log)) == 1, log.text


# ---- destinations and formats ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS[1:], ids=lambda l: l[0])
@pytest.mark.parametrize("cn", (1, 3))
def test_a_batch_of_three_into_pitched_and_offset_destinations(rip_lib, cn, layout):
    """Row padding, the gaps between frames and the bytes in front of an offset base keep their sentinels, around a letterbox with
    bands on either side and around a cropped window."""
    pipe = plain_pipe()
    run_case(pipe, FC.case(cn, (70, 33), (5, 2, 60, 30), (45, 41), "letterbox", "area", FC.PADS[2], n=3), layout=layout, seed=1)
    run_case(pipe, FC.case(cn, (70, 33), (5, 2, 61, 30), (33, 50), "letterbox", "linear", FC.PADS[1], n=3), layout=layout, seed=2)
    run_case(pipe, FC.case(cn, (70, 33), (1, 0, 66, 33), (21, 20), "crop", "linear", n=3), layout=layout, seed=3)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_every_format_behind_a_letterbox(rip_lib, fmt):
    """The pad is a colour of F', in front of the format: padded pixels show the table entry or the grey value of the pad bytes,
    and the converter follows the pad kernel unchanged."""
    pipe = plain_pipe()
    for c in (FC.case(3, (70, 33), (5, 2, 60, 30), (45, 41), "letterbox", "area", FC.PADS[2], n=2), FC.case(3, (33, 21), None, (40, 40), "letterbox", "linear", FC.PADS[1], n=2)):
        log = run_case(pipe, c, fmt, layout=LAYOUTS[1])
        names = [n for n in log.names() if n.startswith(STAGE + ("output_convert",))]
        assert names == expected_names(c) + [OV.KERNEL_OF_FORMAT[fmt]] and log.names()[-len(names):] == names, log.text
        frames = FC.frames(c)
        (left, top, wi, hi) = FC.geometry(c)[1]
        full = want(frames, c, fmt)
        one = R.convert(np.array(c.pad, np.uint8).reshape(1, 1, 1, 3), fmt, *NORM)              # what the format makes of one pad pixel
        corner = full[:, :, 0, 0] if R.is_planar(fmt) else full[:, 0, 0]
        assert (top > 0 or left > 0) and np.array_equal(R.bits(corner), R.bits(np.broadcast_to(one.reshape(corner.shape[1:]), corner.shape)))


def test_mono8_frames_with_a_coloured_pad(rip_lib):
    pipe = plain_pipe()
    for pad in FC.PADS + ((255, 0, 0), (0, 0, 255)):
        for fmt in ("native", "mono8"):
            c = FC.case(1, (33, 21), (1, 1, 30, 19), (40, 37), "letterbox", "linear", pad, n=2)
            log = run_case(pipe, c, fmt)
            assert "output_convert" not in log.text
    assert FR.pad_bytes((0, 255, 7), 1) == (152,) and FR.pad_bytes((201, 33, 90), 1) == (69,)


# ---- behind the real pipeline ------------------------------------------------------------------------------------------------------
BEHIND = (((7, 5, 150, 100), (96, 96), "letterbox", "area"), (None, (64, 64), "crop", "linear"), ((33, 2, 101, 77), None, "stretch", "linear"))


def run_behind(pipe, batch, enc, refs, what, **kw):
    """The batch on one handle under three settings of window, target and fit (BEHIND), native and under a planar format; refs: E
    per frame."""
    import torch
    e = np.stack(refs)
    for k, (roi, target, fit, interp) in enumerate(BEHIND):
        if roi is not None and (roi[0] + roi[2] > e.shape[2] or roi[1] + roi[3] > e.shape[1]):
            roi = (roi[1], roi[0], roi[3], roi[2])                                       # a flipped image: the window flipped too
        c = FC.case(3, (e.shape[2], e.shape[1]), roi, target, fit, interp, FC.PADS[k], n=len(e))
        fmt = ("native", "rgb_chw_f16", "mono8")[k]
        setup(pipe, c, fmt)
        with pipe.launch_log() as log:
            out = pipe.apply_device(batch, enc, **kw)
            torch.cuda.synchronize()
        ref = want(e, c, fmt)
        assert tuple(out.shape) == ref.shape, (what, k, out.shape, ref.shape)
        got = delivered(out)
        assert np.array_equal(got, R.bits(ref)), "%s setting %d: %d of %d elements differ" % (what, k, int((got != R.bits(ref)).sum()), got.size)
        tail = expected_names(c) + ([OV.KERNEL_OF_FORMAT[fmt]] if fmt != "native" else [])
        assert log.names()[-len(tail):] == tail, log.text
        assert pipe.get_output_window(batch.shape[1], kw.get("width", batch.shape[2]), 1, enc) == FC.geometry(c)[:2]


def test_behind_the_full_chain_with_undistortion(rip_lib, oracle):
    import torch
    w, h = V.REMAP_SIZE
    cam = synth.camera_model(w, h)
    c = cfg(cam=cam, undistort=True, flip=True, flip_angle=180, **FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_output_normalization(*NORM)
    frames = bayer_frames(w, h, "grbg")
    refs = [oracle_run(oracle, c, f, "bayer_grbg8")[0] for f in frames]
    run_behind(pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_grbg8", refs, "full chain + undistortion")
    # the camera matrices of what was delivered last: the rect matrices through the window
    roi, target, fit, _ = BEHIND[2]
    hh, ww, k, pr = pipe.get_output_camera_info(h, w, 1, "bayer_grbg8")
    eh, ew, ek, ep = FR.camera(pipe.get_rect_camera_matrix(), pipe.get_rect_projection_matrix(), w, h, roi, target, fit)
    assert (hh, ww) == (eh, ew) and k.tobytes() == ek.tobytes() and pr.tobytes() == ep.tobytes()


def test_behind_flip_90(rip_lib, oracle):
    import torch
    w, h = V.REMAP_SIZE
    c = cfg(flip=True, flip_angle=90, **FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_output_normalization(*NORM)
    frames = bayer_frames(w, h, "gbrg")
    refs = [oracle_run(oracle, c, f, "bayer_gbrg8")[0] for f in frames]
    assert refs[0].shape == (w, h, 3)
    run_behind(pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_gbrg8", refs, "flip 90")


def test_behind_mht(rip_lib, oracle):
    import torch
    w, h = V.REMAP_SIZE
    c = cfg(**FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_output_normalization(*NORM)
    pipe.set_debayer_method("mht")
    frames = bayer_frames(w, h, "bggr")
    refs = [expected_mht(oracle, c, f, "bayer_bggr8")[0] for f in frames]
    run_behind(pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_bggr8", refs, "mht")


def test_behind_a_packed_10_bit_frame(rip_lib, oracle):
    import torch
    w, h = V.REMAP_SIZE
    c = cfg(**FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_output_normalization(*NORM)
    pipe.set_debayer_16bit_range(64, 1023)
    samples = [G.gen_frame16(w, h, "rggb", 70 + i, 64, 1023, kind="random" if i == 1 else "scene").clip(0, 1023).astype(np.uint16) for i in range(3)]
    refs = [expected_raw16(oracle, c, f, "rggb", "bilinear", 64, 1023)[0] for f in samples]
    packed = np.stack([PKR.pack(f, "10p") for f in samples])
    run_behind(pipe, torch.from_numpy(packed).cuda(), PKR.enc("rggb", "10p"), refs, "packed 10p", width=w)


def test_behind_the_chain_under_the_contracted_model(rip_lib, oracle):
    import torch
    w, h = V.REMAP_SIZE
    c = cfg(ce=True, ce_hue=1.3, ce_sat=0.7, ce_val=1.1, **FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    pipe.set_output_normalization(*NORM)
    pipe.set_fp_contraction(1)
    frames = bayer_frames(w, h, "rggb")
    with oracle.fp_contraction(1):
        refs = [oracle_run(oracle, c, f, "bayer_rggb8")[0] for f in frames]
    run_behind(pipe, torch.from_numpy(np.stack(frames)).cuda(), "bayer_rggb8", refs, "chain fc=1")


# ---- state -------------------------------------------------------------------------------------------------------------------------
def test_switching_window_fit_and_target_on_one_handle_between_frames(rip_lib):
    """One table set is kept per handle, keyed by the sizes: the same sizes at another origin, another fit, another window size
    and back again all deliver their own reference."""
    pipe = plain_pipe()
    size = (61, 40)
    seq = [((3, 2, 40, 30), (20, 20), "letterbox", "linear"), ((7, 5, 40, 30), (20, 20), "letterbox", "linear"), ((7, 5, 40, 30), (20, 20), "crop", "linear"),
           ((7, 5, 40, 30), (20, 20), "crop", "area"), (None, (20, 20), "stretch", "area"), ((7, 5, 40, 30), None, "crop", "area"), (None, None, "letterbox", "linear"),
           ((0, 0, 61, 40), (61, 40), "letterbox", "area"), ((3, 2, 40, 30), (20, 20), "letterbox", "linear"), ((1, 1, 40, 30), (20, 15), "stretch", "area")]
    for i, (roi, target, fit, interp) in enumerate(seq):
        for cn in (3, 1):
            run_case(pipe, FC.case(cn, size, roi, target, fit, interp, FC.PADS[i % 3], n=2), seed=i)


def test_ccc_sequence_keeps_its_track_with_a_window_and_a_refused_frame_moves_nothing(rip_lib, oracle):
    """Five frames with temporal consistency on a handle with a window and a letterbox and on a twin without either: the same track,
    the same gains, the same taps; RIP_IMAGE_PROCESSED is empty on the first.  In between, a frame whose geometry puts the window
    outside F is refused by every frame call before anything is enqueued: the track stays the twin's."""
    import torch
    w, h, n = V.CHAIN_SIZE[0], V.CHAIN_SIZE[1], 5
    roi, target = (5, 3, w - 9, h - 4), (w // 2, w // 2)
    filt, bias = synth.ccc_model()
    c = cfg(wb=True, wb_method="ccc", wb_bright=0.8, wb_dark=0.2, wb_temporal=True, gamma=True, gamma_k=0.9)
    pipes = []
    for windowed in (True, False):
        p = RawImagePipeline(False, "", "", "", device=0)
        p.set_ccc_model(filt, bias)
        p.set_ccc_kalman_model(1.0, 10.0)
        configure(p, c)
        p.reset_white_balance_temporal_consistency()
        if windowed:
            p.set_output_roi(*roi)
            p.set_output_size(*target)
            p.set_output_fit("letterbox")
            p.set_output_pad(*FC.PADS[2])
        pipes.append(p)
    occ = oracle.CCC(filt, bias)
    occ.set_kalman_model(1.0, 10.0)
    small = synth.gen_frame(w - 10, h, "bayer_gbrg8", seed=1)
    for i in range(n):
        frame = synth.gen_frame(w, h, "bayer_gbrg8", seed=4100 + i, kind="scene", tint=(0.70 + 0.04 * i, 1.0, 0.55))
        ref = oracle_run(oracle, c, frame, "bayer_gbrg8", ccc=occ)[0]
        got, twin = (p.process(frame, "bayer_gbrg8") for p in pipes)
        assert np.array_equal(twin, ref), "twin without a window, frame %d" % i
        assert np.array_equal(got, FR.expected(ref, roi, target, "letterbox", "linear", FC.PADS[2])), "frame %d" % i
        assert np.array_equal(pipes[0].get_ccc_track(1), pipes[1].get_ccc_track(1))
        assert np.array_equal(pipes[0].get_white_balance_info(1), pipes[1].get_white_balance_info(1))
        for getter in ("get_dist_debayered_image", "get_dist_color_image"):
            a, b = getattr(pipes[0], getter)(), getattr(pipes[1], getter)()
            assert a.shape == (h, w, 3) and np.array_equal(a, b), getter
        assert pipes[0].get_processed_image().size == 0 and np.array_equal(pipes[1].get_processed_image(), ref)
        if i == 2:
            batch = torch.from_numpy(np.stack([small, small])).cuda()
            with pipes[0].launch_log() as log:
                for call in (lambda: pipes[0].process(small, "bayer_gbrg8"), lambda: pipes[0].submit(small, "bayer_gbrg8"),
                             lambda: pipes[0].apply_device(batch, "bayer_gbrg8"), lambda: pipes[0].query_output(h, w - 10, 1, "bayer_gbrg8")):
                    with pytest.raises(ValueError) as e:
                        call()
                    assert "does not lie inside" in str(e.value)
            assert not log.records(), log.text


@pytest.mark.parametrize("fmt", ("native", "rgb_chw_f16"))
def test_host_paths(rip_lib, oracle, fmt):
    """rip_apply, submit / collect and a pinned destination deliver the letterboxed window; capacities are the delivered frame's;
    RIP_IMAGE_PROCESSED is empty, with a window and no target too."""
    w, h = 37, 29
    c = cfg(**FULL)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, c)
    k = FC.case(3, (w, h), (2, 3, 33, 20), (24, 30), "letterbox", "area", FC.PADS[1])
    setup(pipe, k, fmt)
    pipe.set_output_normalization(*NORM)
    frames = bayer_frames(w, h, "rggb", 3)
    refs = [oracle_run(oracle, c, f, "bayer_rggb8")[0] for f in frames]
    wants = [want(e[None], k, fmt)[0] for e in refs]

    def same(got, i, what):
        assert got.shape == wants[i].shape and got.dtype == wants[i].dtype, (what, got.shape, got.dtype)
        assert np.array_equal(R.bits(got), R.bits(wants[i])), "%s %s" % (fmt, what)
    same(pipe.process(frames[0], "bayer_rggb8"), 0, "process")
    assert pipe.get_processed_image().size == 0
    assert pipe.get_dist_debayered_image().shape == (h, w, 3) and pipe.get_dist_color_image().shape == (h, w, 3)
    t = [pipe.submit(f, "bayer_rggb8") for f in frames[:2]]
    same(pipe.collect(t[0]), 0, "collect copy")
    same(pipe.collect(t[1], copy=False), 1, "collect view")
    nbytes, elem, planar = pipe.query_output_bytes(h, w, 1, "bayer_rggb8")
    assert nbytes == wants[0].nbytes and elem == wants[0].itemsize and planar == (fmt == "rgb_chw_f16")
    pinned = P.host_alloc(wants[2].shape, wants[2].dtype)
    pinned.view(np.uint8)[...] = SENTINEL
    assert pipe.collect(pipe.submit(frames[2], "bayer_rggb8", out=pinned)) is pinned
    same(pinned, 2, "submit into a pinned array")
    small = P.host_alloc((nbytes - 1,), np.uint8)
    small[...] = SENTINEL
    f = np.ascontiguousarray(frames[0])
    with pipe.launch_log() as log:
        r, cc, kk = C.c_int(), C.c_int(), C.c_int()
        st = pipe._lib.rip_apply(pipe._h, f.ctypes.data_as(C.c_void_p), h, w, 1, C.c_size_t(w), b"bayer_rggb8", small.ctypes.data_as(C.c_void_p),
                                 C.c_size_t(small.nbytes), C.byref(r), C.byref(cc), C.byref(kk), None)
        assert st == P.RIP_ERR_CAPACITY
    assert not log.records() and (small == SENTINEL).all()
    # a window and no target: the window itself, and still no processed image
    pipe.set_output_size(0, 0)
    pipe.set_output_format("native")
    got = pipe.process(frames[1], "bayer_rggb8")
    assert np.array_equal(got, refs[1][3:23, 2:35]) and pipe.get_processed_image().size == 0
    pipe.set_output_roi(0, 0, 0, 0)
    got = pipe.process(frames[2], "bayer_rggb8")
    assert np.array_equal(got, refs[2]) and np.array_equal(pipe.get_processed_image(), refs[2])


# ---- the launch log -----------------------------------------------------------------------------------------------------------------
def test_defaults_and_a_window_equal_to_f_log_what_a_handle_without_the_settings_logs(rip_lib, oracle):
    """Per format and target: a handle that never heard of the settings, one with the defaults set explicitly and another pad, and
    one whose window is all of F under "stretch" log the same launches and deliver the same bytes; none is a kernel of
    librip_fit_hip.so.  Without a target the window equal to F launches no resize at all."""
    import torch
    w, h = V.REMAP_SIZE
    frames = bayer_frames(w, h, "rggb")
    batch = torch.from_numpy(np.stack(frames)).cuda()
    cam = synth.camera_model(w, h)
    c = cfg(cam=cam, undistort=True, **FULL)
    for fmt in ("native", "rgb_chw_f16"):
        for target in ((0, 0), (w, h), (w // 2, h // 2), (w // 2 + 1, h // 2 + 1)):
            for interp in ("linear", "area"):
                logs, outs = [], []
                for variant in ("untouched", "defaults", "window"):
                    pipe = RawImagePipeline(False, "", "", "", device=0)
                    configure(pipe, c)
                    pipe.set_output_format(fmt)
                    pipe.set_output_size(*target)
                    pipe.set_output_interpolation(interp)
                    if variant != "untouched":
                        pipe.set_output_roi(*((0, 0, 0, 0) if variant == "defaults" else (0, 0, w, h)))
                        pipe.set_output_fit("stretch")
                        pipe.set_output_pad(1, 2, 3)
                    with pipe.launch_log() as log:
                        outs.append(delivered(pipe.apply_device(batch, "bayer_rggb8")))
                        torch.cuda.synchronize()
                    logs.append(log.text)
                assert logs[0] == logs[1] == logs[2] and "fit_" not in logs[0], (fmt, target, interp)
                assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
                if target in ((0, 0), (w, h)):
                    assert not [ln for ln in logs[0].splitlines() if ln.startswith(STAGE)]


# ---- a seeded fuzz ----------------------------------------------------------------------------------------------------------------
FUZZ_CASES = 40
FUZZ_FORMATS = ("native",) + R.FORMATS


def fuzz_case(seed):
    """Draws accepted configurations only: the window lies inside F, and under "area" a draw that would enlarge the window on an
    axis is made again with the target shrunk to the picture's limits."""
    rng = np.random.default_rng(77000 + seed)
    cn = int(rng.choice([1, 3]))
    fmt = FUZZ_FORMATS[int(rng.integers(len(FUZZ_FORMATS)))] if cn == 3 else ("native", "mono8")[int(rng.integers(2))]
    C_, R_ = (int(v) for v in rng.integers(1, 90, 2))
    roi = None
    if rng.random() < 0.8:
        w, h = int(rng.integers(1, C_ + 1)), int(rng.integers(1, R_ + 1))
        roi = (int(rng.integers(0, C_ - w + 1)), int(rng.integers(0, R_ - h + 1)), w, h)
    fit = FR.FITS[int(rng.integers(3))]
    interp = ("linear", "area")[int(rng.integers(2))]
    target = None
    if rng.random() < 0.85:
        target = tuple(int(v) for v in rng.integers(1, 90, 2))
        if rng.random() < 0.2:
            ws, hs = (roi or (0, 0, C_, R_))[2:]
            target = (max(1, ws // 2), max(1, hs // 2))                   # often the 2 x 2 mean
        if interp == "area":
            for _ in range(8):                                           # shrink until window -> picture is a downscale
                src, dst, _ = FR.geometry(C_, R_, roi, target, fit)
                if dst[2] <= src[2] and dst[3] <= src[3]:
                    break
                target = (max(1, min(target[0], src[2]) - (dst[2] > src[2])), max(1, min(target[1], src[3]) - (dst[3] > src[3])))
            src, dst, _ = FR.geometry(C_, R_, roi, target, fit)
            if dst[2] > src[2] or dst[3] > src[3]:
                interp = "linear"
    pad = tuple(int(v) for v in rng.integers(0, 256, 3))
    return FC.case(cn, (C_, R_), roi, target, fit, interp, pad, n=int(rng.integers(1, 5))), fmt, LAYOUTS[int(rng.integers(3))]


@pytest.mark.parametrize("seed", range(FUZZ_CASES))
def test_fuzz(rip_lib, seed):
    c, fmt, layout = fuzz_case(seed)
    pipe = plain_pipe()
    log = run_case(pipe, c, fmt, layout=layout, seed=seed)
    names = [n for n in log.names() if n.startswith("output_convert")]
    assert len(names) == (0 if fmt == "native" or c.channels == 1 else 1), log.text


def test_the_fuzz_draws_every_fit_interpolation_and_kind_of_band():
    draws = [fuzz_case(s)[0] for s in range(FUZZ_CASES)]
    assert {c.fit for c in draws} == set(FR.FITS) and {c.interpolation for c in draws} == {"linear", "area"} and {c.channels for c in draws} == {1, 3}
    assert any(c.roi is None for c in draws) and any(c.target is None for c in draws)
    kernels = {FC.kernel_of(c)[0].split("<")[0] for c in draws}
    assert {"fit_linear_kernel", "fit_area_kernel"} <= kernels
    assert any(FC.kernel_of(c)[1] for c in draws)
