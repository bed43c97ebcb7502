"""The window and the fit modes of the resize stage (include/rip.h rip_set_output_roi, rip_set_output_fit, rip_set_output_pad)
without a GPU: the host's geometry against tests/fit_reference.py for every small quadruple of sides and the known answers of
PARITY.md "Resize: window and fit", its properties, the setters and getters, the YAML keys, the queries and the camera matrices on
RIP_DEVICE_NONE handles, the refusals and their order, the C++ facade, and the kernels of csrc/rip_fit.hip executed on the host
against the reference.  Everything at tolerance 0."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import fit_cases as FC
import fit_reference as FR
import resize_reference as Z
from helpers import CSRC, build_host_program
from raw_image_pipeline_amd import pipeline as P
from test_cpp_facade import BRANCHES, run_env
from test_resize import neutral, write_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = P.RIP_ERR_INVALID_ARGUMENT
LARGE = ((2448, 2048, 640, 480), (2448, 2048, 224, 224), (2448, 2048, 1, 1), (2448, 2048, 16384, 3), (640, 480, 2448, 2048), (16384, 3, 3, 16384),
         (16384, 16384, 1, 16384), (1, 16384, 16384, 1))
CALLS = ("query_output", "query_output_bytes", "get_output_camera_info", "get_output_window")


def hook(lib, C_, R_, roi, target, fit):
    src, dst = (C.c_int * 4)(*([-7] * 4)), (C.c_int * 4)(*([-7] * 4))
    st = lib.rip_debug_output_window(C_, R_, (C.c_int * 4)(*(roi or (0, 0, 0, 0))), target[0], target[1], fit.encode(), src, dst)
    return st, tuple(src), tuple(dst)


# ---- the geometry ----------------------------------------------------------------------------------------------------------
def test_host_geometry_equals_the_reference_for_every_quadruple_of_small_sides(rip_lib):
    """Every (w, h, W, H) with sides in 1..24, all three fit modes, the window being all of F."""
    fn = rip_lib.rip_debug_output_window
    src, dst, roi = (C.c_int * 4)(), (C.c_int * 4)(), (C.c_int * 4)(0, 0, 0, 0)
    names = {f: f.encode() for f in FR.FITS}
    for w in range(1, 25):
        for h in range(1, 25):
            for W in range(1, 25):
                for H in range(1, 25):
                    for fit in FR.FITS:
                        assert fn(w, h, roi, W, H, names[fit], src, dst) == P.RIP_OK
                        assert (tuple(src), tuple(dst)) == FR.geometry(w, h, None, (W, H), fit)[:2], (w, h, W, H, fit)


@pytest.mark.parametrize("w,h,W,H", LARGE)
def test_host_geometry_equals_the_reference_for_large_sides(rip_lib, w, h, W, H):
    for fit in FR.FITS:
        for roi, size in ((None, (w, h)), ((5, 3, w, h), (w + 9, h + 3)), ((0, 7, w, h), (w, h + 7))):
            st, src, dst = hook(rip_lib, size[0], size[1], roi, (W, H), fit)
            assert st == P.RIP_OK and (src, dst) == FR.geometry(size[0], size[1], roi, (W, H), fit)[:2], (fit, roi)


def test_known_answers(rip_lib):
    assert FR.geometry(2448, 2048, None, (640, 480), "crop") == ((0, 106, 2448, 1836), (0, 0, 640, 480), (640, 480))
    assert FR.geometry(2448, 2048, None, (640, 480), "letterbox") == ((0, 0, 2448, 2048), (33, 0, 574, 480), (640, 480))
    assert hook(rip_lib, 2448, 2048, None, (640, 480), "crop") == (P.RIP_OK, (0, 106, 2448, 1836), (0, 0, 640, 480))
    assert hook(rip_lib, 2448, 2048, None, (640, 480), "letterbox") == (P.RIP_OK, (0, 0, 2448, 2048), (33, 0, 574, 480))
    assert hook(rip_lib, 2448, 2048, None, (640, 480), "stretch") == (P.RIP_OK, (0, 0, 2448, 2048), (0, 0, 640, 480))
    assert hook(rip_lib, 2448, 2048, (8, 4, 100, 50), (0, 0), "letterbox") == (P.RIP_OK, (8, 4, 100, 50), (0, 0, 100, 50))   # no target: the fit has no effect
    assert FR.pad_bytes((114, 114, 114), 1) == (114,) and FR.pad_bytes((255, 0, 0), 1) == (29,) and FR.pad_bytes((0, 255, 0), 1) == (150,)
    assert FR.pad_bytes((0, 0, 255), 1) == (76,) and FR.pad_bytes((255, 255, 255), 1) == (255,)


def test_geometry_properties():
    """The picture lies inside the target; crop's window lies inside the given window, centred, with the other side kept; equal
    aspects reduce both modes to stretch; letterbox keeps the whole window and binds one side."""
    rng = np.random.default_rng(5)
    draws = [tuple(int(v) for v in rng.integers(1, 400, 4)) for _ in range(3000)] + [(w, h, W, H) for w in (1, 2, 7) for h in (1, 3, 8) for W in (1, 5) for H in (1, 4)]
    for (w, h, W, H) in draws:
        x, y = int(rng.integers(0, 9)), int(rng.integers(0, 9))
        roi, size = (x, y, w, h), (x + w + 2, y + h + 1)
        stretch = FR.geometry(size[0], size[1], roi, (W, H), "stretch")
        assert stretch == (roi, (0, 0, W, H), (W, H))
        (cx, cy, cw, ch), cdst, _ = FR.geometry(size[0], size[1], roi, (W, H), "crop")
        assert cdst == (0, 0, W, H) and 1 <= cw <= w and 1 <= ch <= h and (cw == w or ch == h)
        assert x <= cx and cx + cw <= x + w and y <= cy and cy + ch <= y + h
        assert (cx - x) in ((w - cw) // 2,) and (cy - y) == (h - ch) // 2
        lsrc, (left, top, wi, hi), _ = FR.geometry(size[0], size[1], roi, (W, H), "letterbox")
        assert lsrc == roi and 1 <= wi <= W and 1 <= hi <= H and (wi == W or hi == H)
        assert 0 <= left and left + wi <= W and 0 <= top and top + hi <= H
        assert left == (W - wi) // 2 and top == (H - hi) // 2 and (W - wi - left) - left in (0, 1) and (H - hi - top) - top in (0, 1)
        if w * H == h * W:
            assert (cx, cy, cw, ch) == roi and (left, top, wi, hi) == (0, 0, W, H)


# ---- the parameter surface -------------------------------------------------------------------------------------------------
def test_defaults_set_get_and_reject(host_pipe):
    p = host_pipe
    lib = p._lib
    assert p.get_output_roi() == (0, 0, 0, 0) and p.get_output_fit() == "stretch" and p.get_output_pad() == (114, 114, 114)
    for roi in ((0, 0, 1, 1), (5, 7, 16384, 16384), (100000, 3, 2, 9), (0, 0, 0, 0), (3, 4, 5, 6)):
        p.set_output_roi(*roi)
        assert p.get_output_roi() == roi
    for bad in ((-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (1, 0, 0, 0), (0, 0, 16385, 4), (0, 0, 4, 16385), (0, 0, -4, 4)):
        with pytest.raises(ValueError) as e:
            p.set_output_roi(*bad)
        assert "1..16384" in str(e.value)
        assert p.get_output_roi() == (3, 4, 5, 6)
    for name in ("letterbox", "crop", "stretch", "letterbox"):
        p.set_output_fit(name)
        assert p.get_output_fit() == name
    for bad in ("", "Letterbox", "CROP", "fill", "pad", "crop ", "contain"):
        with pytest.raises(ValueError) as e:
            p.set_output_fit(bad)
        assert '"stretch", "letterbox" or "crop"' in str(e.value)
        assert p.get_output_fit() == "letterbox"
    for pad in ((0, 0, 0), (255, 255, 255), (1, 2, 3)):
        p.set_output_pad(*pad)
        assert p.get_output_pad() == pad
    for bad in ((-1, 0, 0), (0, 256, 0), (0, 0, 1000), (256, 256, 256)):
        with pytest.raises(ValueError) as e:
            p.set_output_pad(*bad)
        assert "0..255" in str(e.value)
        assert p.get_output_pad() == (1, 2, 3)
    assert lib.rip_set_output_roi(None, 0, 0, 1, 1) == INVALID and lib.rip_set_output_fit(None, b"crop") == INVALID
    assert lib.rip_set_output_fit(p._h, None) == INVALID and lib.rip_set_output_pad(None, 1, 1, 1) == INVALID
    buf = C.create_string_buffer(4)
    assert lib.rip_get_output_fit(p._h, buf, C.c_size_t(4)) != P.RIP_OK                      # no room for the name
    assert lib.rip_get_output_roi(p._h, None, None, None, None) == P.RIP_OK and lib.rip_get_output_pad(p._h, None, None, None) == P.RIP_OK
    assert lib.rip_get_output_window(p._h, 30, 44, 3, b"bgr8", None, None) == P.RIP_OK
    assert lib.rip_get_output_window(p._h, 30, 44, 3, None, None, None) == INVALID


def test_the_debug_hook_refuses_what_the_setters_refuse(rip_lib):
    for args in ((0, 4, None, (2, 2), "crop"), (4, 0, None, (2, 2), "crop"), (8, 8, (0, 0, 0, 3), (2, 2), "crop"), (8, 8, (-1, 0, 2, 2), (2, 2), "crop"),
                 (8, 8, None, (0, 2), "crop"), (8, 8, None, (16385, 2), "crop"), (8, 8, None, (2, 2), "fill"), (8, 8, (7, 0, 2, 2), (2, 2), "crop"),
                 (8, 8, (0, 7, 2, 2), (0, 0), "stretch")):
        assert hook(rip_lib, *args)[0] == INVALID, args
    assert rip_lib.rip_debug_output_window(8, 8, None, 2, 2, b"crop", (C.c_int * 4)(), (C.c_int * 4)()) == INVALID
    assert hook(rip_lib, 8, 8, (6, 6, 2, 2), (0, 0), "stretch") == (P.RIP_OK, (6, 6, 2, 2), (0, 0, 2, 2))                  # the window ends with F


def test_yaml_keys(tmp_path, host_pipe):
    p = host_pipe
    p.load_params(write_params(tmp_path, "output:\n  size: [640, 480]\n  roi: [8, 4, 2000, 1000]\n  fit: letterbox\n  pad: [0, 128, 255]\n"))
    assert (p.get_output_roi(), p.get_output_fit(), p.get_output_pad(), p.get_output_size()) == ((8, 4, 2000, 1000), "letterbox", (0, 128, 255), (640, 480))
    p.load_params(write_params(tmp_path, "output:\n  size: [640, 480]\n"))                    # absent: the defaults
    assert (p.get_output_roi(), p.get_output_fit(), p.get_output_pad()) == ((0, 0, 0, 0), "stretch", (114, 114, 114))
    p.load_params(write_params(tmp_path, "output:\n  fit: crop\n  roi: [0, 0, 0, 0]\n"))
    assert p.get_output_fit() == "crop" and p.get_output_roi() == (0, 0, 0, 0)
    p.set_output_roi(1, 2, 3, 4)
    p.set_output_pad(9, 9, 9)
    p.load_params(write_params(tmp_path, "debayer:\n  enabled: true\n"))                      # rip_load_params re-creates the modules
    assert (p.get_output_roi(), p.get_output_fit(), p.get_output_pad()) == ((0, 0, 0, 0), "stretch", (114, 114, 114))


@pytest.mark.parametrize("bad", ["fit: fill", "fit: Crop", "fit: [crop]", "fit: ''", "roi: [0, 0, 4]", "roi: [0, 0, 0, 4]", "roi: [-1, 0, 4, 4]", "roi: [0, 0, 4.5, 4]",
                                 "roi: [0, 0, 16385, 4]", "roi: 7", "pad: [0, 0]", "pad: [0, 0, 256]", "pad: [-1, 0, 0]", "pad: [1.5, 0, 0]", "pad: grey"])
def test_yaml_invalid_value_fails_and_changes_nothing(tmp_path, host_pipe, bad):
    p = host_pipe
    p.set_output_size(33, 17)
    p.set_output_roi(1, 2, 30, 40)
    p.set_output_fit("crop")
    p.set_output_pad(7, 8, 9)
    p.set_output_format("bgr_chw_f32")
    p.set_flip(True)
    with pytest.raises(ValueError):
        p.load_params(write_params(tmp_path, "output:\n  size: [8, 8]\n  %s\n  format: rgb8\nflip:\n  enabled: false\n" % bad))
    assert (p.get_output_roi(), p.get_output_fit(), p.get_output_pad()) == ((1, 2, 30, 40), "crop", (7, 8, 9))
    assert p.get_output_size() == (33, 17) and p.get_output_format() == "bgr_chw_f32" and p.is_flip_enabled()


# ---- queries and camera matrices -------------------------------------------------------------------------------------------
CONFIGS = [(roi, target, fit) for roi in (None, (0, 0, 64, 48), (5, 3, 40, 21), (63, 47, 1, 1), (1, 0, 63, 48))
           for target in (None, (64, 48), (32, 24), (17, 9), (100, 100), (1, 1), (20, 40)) for fit in FR.FITS]


def test_queries_and_camera_matrices_equal_the_reference(host_pipe):
    """rip_query_output, rip_query_output_bytes, rip_get_output_window and rip_get_output_camera_info for a 64 x 48 frame: the
    delivered geometry and both rectangles are the reference's, the matrices equal its Python floats bit for bit (==), with and
    without undistortion (rect / dist matrices), under every format's geometry."""
    from raw_image_pipeline_amd import synth
    p = host_pipe
    neutral(p)
    synth.load_camera(p, synth.camera_model(64, 48))
    for und in (False, True):
        p.set_undistortion(und)
        K = np.array(p.get_rect_camera_matrix() if und else p.get_dist_camera_matrix(), np.float64)
        Pm = np.array(p.get_rect_projection_matrix() if und else p.get_dist_projection_matrix(), np.float64)
        for fmt, channels, elem, planar in (("native", 3, 1, 0), ("mono8", 1, 1, 0), ("rgb_chw_f16", 3, 2, 1)):
            p.set_output_format(fmt)
            for roi, target, fit in CONFIGS:
                p.set_output_roi(*(roi or (0, 0, 0, 0)))
                p.set_output_size(*(target or (0, 0)))
                p.set_output_fit(fit)
                src, dst, (W, H) = FR.geometry(64, 48, roi, target, fit)
                what = (und, fmt, roi, target, fit)
                assert p.get_output_window(48, 64, 1, "bayer_rggb8") == (src, dst), what
                assert p.query_output(48, 64, 1, "bayer_rggb8")[:3] == (H, W, channels), what
                assert p.query_output_bytes(48, 64, 1, "bayer_rggb8") == (H * W * channels * elem, elem, planar), what
                assert p.query_taps(48, 64, 1, "bayer_rggb8") == (48, 64, 3), what
                h, w, k, pr = p.get_output_camera_info(48, 64, 1, "bayer_rggb8")
                eh, ew, ek, ep = FR.camera(K, Pm, 64, 48, roi, target, fit)
                assert (h, w) == (eh, ew) and k.tobytes() == ek.tobytes() and pr.tobytes() == ep.tobytes(), what


def test_the_defaults_keep_the_camera_matrices_of_the_plain_resize(host_pipe):
    """Window off and "stretch": rip_get_output_camera_info takes the path it took before there was a window -- bit-equal to
    tests/resize_reference.py's scaled_camera, the formula of PARITY.md "Resize" -- whatever pad colour is set."""
    from raw_image_pipeline_amd import synth
    p = host_pipe
    neutral(p)
    synth.load_camera(p, synth.camera_model(64, 48))
    p.set_output_pad(1, 2, 3)
    K, Pm = np.array(p.get_dist_camera_matrix(), np.float64), np.array(p.get_dist_projection_matrix(), np.float64)
    for target in ((0, 0), (64, 48), (32, 24), (17, 9), (100, 100), (1, 1), (21, 48), (640, 7)):
        p.set_output_size(*target)
        h, w, k, pr = p.get_output_camera_info(48, 64, 1, "bayer_rggb8")
        H, W = (target[1], target[0]) if target != (0, 0) else (48, 64)
        ek, ep = Z.scaled_camera(K, Pm, 48, 64, H, W)
        assert (h, w) == (H, W) and k.tobytes() == ek.tobytes() and pr.tobytes() == ep.tobytes(), target
        assert p.get_output_window(48, 64, 1, "bayer_rggb8") == ((0, 0, 64, 48), (0, 0, W, H))


def test_a_flip_by_90_degrees_swaps_the_sides_the_window_is_checked_against(host_pipe):
    p = host_pipe
    neutral(p)
    p.set_output_roi(0, 0, 48, 64)
    with pytest.raises(ValueError):
        p.query_output(48, 64, 3, "bgr8")
    p.set_flip(True)
    p.set_flip_angle(90)
    assert p.query_output(48, 64, 3, "bgr8")[:2] == (64, 48)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def refused(p, word, *frame):
    for call in CALLS:
        with pytest.raises(ValueError) as e:
            getattr(p, call)(*frame)
        assert word in str(e.value), (call, str(e.value))


def test_refusals_and_their_order(host_pipe):
    p = host_pipe
    neutral(p)
    frame = (30, 44, 3, "bgr8")
    # a window outside F: x + width > C or y + height > R, by one pixel; touching the edge is fine
    for roi, ok in (((4, 0, 40, 30), True), ((5, 0, 40, 30), False), ((0, 1, 44, 30), False), ((43, 29, 1, 1), True), ((44, 0, 1, 1), False), ((0, 30, 1, 1), False),
                    ((0, 0, 16384, 1), False), ((4000000, 0, 1, 1), False)):
        p.set_output_roi(*roi)
        for target in ((0, 0), (8, 8)):
            p.set_output_size(*target)
            for fit in FR.FITS:
                p.set_output_fit(fit)
                if ok:
                    assert p.get_output_window(*frame)[0][2:] <= roi[2:]
                else:
                    refused(p, "does not lie inside", *frame)
    # under "area" the upscale and factor rules look at window size -> picture size
    p.set_output_interpolation("area")
    p.set_output_fit("stretch")
    p.set_output_roi(2, 2, 20, 10)
    p.set_output_size(20, 10)
    assert p.query_output(*frame)[:2] == (10, 20)                       # the copy of the window
    p.set_output_size(21, 10)
    refused(p, "downscale", *frame)
    p.set_output_size(44, 30)                                           # F's size, yet an upscale of the window
    refused(p, "downscale", *frame)
    p.set_output_fit("letterbox")                                       # picture 44 x 22 of a 20 x 10 window
    refused(p, "downscale", *frame)
    p.set_output_roi(0, 0, 0, 0)
    p.set_output_size(60, 30)                                           # picture 44 x 30 at left = 8: the copy of F between two bands
    assert p.get_output_window(*frame) == ((0, 0, 44, 30), (8, 0, 44, 30)) and p.query_output(*frame)[:2] == (30, 60)
    p.set_output_size(1, 1)
    p.set_output_fit("crop")
    p.set_output_interpolation("linear")
    assert p.get_output_window(300, 1000, 1, "mono8") == ((350, 0, 300, 300), (0, 0, 1, 1))
    p.set_output_interpolation("area")
    refused(p, "256", 300, 1000, 1, "mono8")                            # 300 > 256 x 1 after the crop too
    p.set_output_roi(0, 0, 1000, 256)
    assert p.query_output(300, 1000, 1, "mono8")[:2] == (1, 1)          # crop: 256 x 256 -> 1 x 1
    p.set_output_fit("stretch")
    refused(p, "256", 300, 1000, 1, "mono8")
    p.set_output_interpolation("linear")
    assert p.query_output(300, 1000, 1, "mono8")[:2] == (1, 1)
    # the order: bgr16 first, then the window outside F, then an F above 16384, then the area rules
    p.set_debayer_16bit(True)
    p.set_output_interpolation("area")
    p.set_output_size(0, 0)
    p.set_output_roi(0, 0, 100, 100)
    refused(p, "bgr16", 30, 44, 1, "bayer_rggb16")                      # also outside F: bgr16 is named
    p.set_output_roi(0, 0, 10, 10)
    refused(p, "bgr16", 30, 44, 1, "bayer_rggb16")                      # a window without a target needs 8 bits too
    p.set_debayer_16bit(False)
    p.set_output_roi(0, 0, 10, 80)
    p.set_output_size(11, 11)
    refused(p, "does not lie inside", 64, 16385, 1, "mono8")            # also too wide an F, also an upscale
    p.set_output_roi(0, 0, 10, 10)
    refused(p, "16384", 64, 16385, 1, "mono8")                          # also an upscale
    refused(p, "downscale", 64, 16384, 1, "mono8")
    p.set_output_size(5, 5)
    assert p.query_output(64, 16384, 1, "mono8")[:2] == (5, 5)
    # the format rules are untouched
    p.set_output_format("rgb8")
    refused(p, "three-channel", 64, 64, 1, "mono8")


def test_all_of_f_as_the_window_is_the_identity(host_pipe):
    p = host_pipe
    neutral(p)
    for fit in FR.FITS:
        p.set_output_fit(fit)
        p.set_output_roi(0, 0, 44, 30)
        for target in ((0, 0), (44, 30)):
            p.set_output_size(*target)
            assert p.query_output(30, 44, 3, "bgr8") == (30, 44, 3, "bgr8")
            assert p.get_output_window(30, 44, 3, "bgr8") == ((0, 0, 44, 30), (0, 0, 44, 30))
    p.set_debayer_16bit(True)                       # fit alone, without a target or a window, refuses nothing
    p.set_output_roi(0, 0, 0, 0)
    p.set_output_size(0, 0)
    assert p.query_output(30, 44, 1, "bayer_rggb16")[3] == "bgr16"


def test_frame_calls_need_a_device_with_a_window_too(host_pipe):
    host_pipe.set_output_roi(0, 0, 4, 4)
    with pytest.raises(P.RipError):
        host_pipe.process(np.zeros((8, 8), np.uint8), "bayer_rggb8")


# ---- C++ facade ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade_sets_gets_and_throws(tmp_path, rip_lib, branch):
    exe = str(tmp_path / ("fit_test_" + branch.replace("-", "_")))
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror"] + BRANCHES[branch] + ["-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "fit_test.cpp"), "-o", exe, "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir,
           "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=run_env(-1))
    assert r.returncode == 0 and "fit host OK" in r.stdout, r.stdout + r.stderr


# ---- the kernels, executed on the host -----------------------------------------------------------------------------------------
LAYOUTS = ((0, 0, 0), (5, 1, 3), (16, 3, 0))      # (row padding, offset of the base, gap between frames) of the destination


# A window that is all of F -- origin (0, 0), F's size -- through the window kernels, which the library never does (it sends such a
# resize to the whole-frame kernels): the one point at which both settings of the bodies' window switch must give the same bytes.
# One shape per arithmetic, a few dozen pixels, the picture's width no multiple of a lane's 4 pixels.
WHOLE_FRAME = {"linear": ("linear", (37, 23), (22, 13)), "mean2": ("linear", (42, 26), (21, 13)), "whole": ("area", (63, 36), (21, 12)),
               "taps": ("area", (37, 23), (22, 13))}


def whole_frame_cases():
    return [FC.case(cn, size, None, target, "stretch", interp) for _, (interp, size, target) in sorted(WHOLE_FRAME.items()) for cn in (1, 3)]


def host_cases():
    """Every shape of tests/fit_cases.py -- the ones the GPU tests run -- and the whole-frame windows above, each under one of three
    destination layouts, two frames."""
    return [(c._replace(n=2), LAYOUTS[i % 3]) for i, c in enumerate(FC.kernel_cases() + whole_frame_cases())]


def test_the_whole_frame_cases_take_the_four_paths():
    for name, (interp, size, target) in WHOLE_FRAME.items():
        assert FR.rule(size, target, interp) == name
    for c in whole_frame_cases():
        assert FC.geometry(c)[:2] == ((0, 0) + c.size, (0, 0) + c.target) and c.target[0] % 4


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_kernels_run_on_the_host_equal_the_reference_byte_for_byte(tmp_path, rip_lib, sanitize):
    """tests/cpp/fit_kernel_host.cpp: csrc/rip_fit.hip compiled as host code with the toolchain's clang++ (-ffp-contract=off), every
    thread of the launchers' grids run in turn from an exactly sized staging image into exactly sized buffers with sentinels,
    tables in exactly sized heap blocks; the geometry is the reference's.  Every byte of the destination is compared: picture,
    bands, row padding, gaps.  The second build adds -fsanitize=address,undefined to this stand-alone program (no
    access outside F or the destination, no misaligned wide access)."""
    exe = build_host_program(tmp_path, "fit_kernel_host", ["fit_kernel_host.cpp", os.path.join(CSRC, "rip_output_tables.cpp")], sanitize=sanitize,
                             extra=["-ffp-contract=off", "-lm", "-lpthread"])
    cases = host_cases()
    assert len(cases) >= 200
    cases_path, out_path = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    frames_of = []
    with open(cases_path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c, (rowpad, off, gap) in cases:
            (xs, ys, ws, hs), (left, top, wi, hi), (W, H) = FC.geometry(c)
            frames = FC.frames(c)
            frames_of.append(frames)
            pad = FR.pad_bytes(c.pad, c.channels) + (0, 0)
            f.write(struct.pack("<21i", c.size[1], c.size[0], c.channels, c.n, xs, ys, ws, hs, wi, hi, int(c.interpolation == "area"), W, H, left, top,
                                rowpad, off, gap, *pad[:3]))
            f.write(frames.tobytes())
    r = subprocess.run([exe, cases_path, out_path], capture_output=True, text=True)
    assert r.returncode == 0 and "%d cases, 0 bad" % len(cases) in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.fromfile(out_path, np.uint8)
    at = 0
    for (c, (rowpad, off, gap)), frames in zip(cases, frames_of):
        (W, H), cn = FC.geometry(c)[2], c.channels
        step = W * cn + rowpad
        frame = step * H + gap
        total = off + frame * (c.n - 1) + step * (H - 1) + W * cn
        want = np.full(total, 0xA5, np.uint8)
        for k in range(c.n):
            image = FR.expected(frames[k], c.roi, c.target, c.fit, c.interpolation, c.pad).reshape(H, W * cn)
            for y in range(H):
                o = off + k * frame + y * step
                want[o:o + W * cn] = image[y]
        assert np.array_equal(got[at:at + total], want), "%s: %d bytes differ" % (FC.case_id(c), int((got[at:at + total] != want).sum()))
        at += total
    assert at == got.size
