"""The resize stage (include/rip.h rip_set_output_size) without a GPU: the host-built tables against tests/resize_reference.py
entry for entry, that reference against oracle.resize_linear byte for byte, validation, the YAML key, the geometry queries and
the camera matrices on RIP_DEVICE_NONE handles and the C++ facade."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import output_reference as R
import resize_reference as Z
from raw_image_pipeline_amd import pipeline as P
from helpers import CSRC, HOST_SANITIZE, build_host_program, host_clangxx
from raw_image_pipeline_amd import synth
from test_cpp_facade import BRANCHES, run_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = P.RIP_ERR_INVALID_ARGUMENT
LARGE_PAIRS = ((2448, 640), (640, 2448), (3, 16384), (16384, 3), (2048, 1024), (2050, 1025))


def hook(lib, R_, C_, H, W):
    xofs, alpha = np.full(W, -7, np.int32), np.full((W, 2), -7, np.int16)
    yofs, beta = np.full((H, 2), -7, np.int32), np.full((H, 2), -7, np.int16)
    area2 = C.c_int(-1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    st = lib.rip_debug_resize_tables(R_, C_, H, W, ptr(xofs), ptr(alpha), ptr(yofs), ptr(beta), C.byref(area2))
    return st, dict(xofs=xofs, alpha=alpha, yofs=yofs, beta=beta, area2=area2.value)


def assert_tables(lib, R_, C_, H, W):
    st, got = hook(lib, R_, C_, H, W)
    assert st == P.RIP_OK, (R_, C_, H, W)
    want = Z.tables(R_, C_, H, W)
    for key in ("xofs", "alpha", "yofs", "beta"):
        assert np.array_equal(got[key], want[key]), "%s of %d x %d -> %d x %d" % (key, R_, C_, H, W)
    assert got["area2"] == want["area2"]


# ---- the tables ------------------------------------------------------------------------------------------------------------
def test_host_tables_equal_the_reference_for_every_pair_of_small_sides(rip_lib):
    """All (src, dst) in 1..40 on the x axis (rows fixed) and on the y axis (columns fixed): the two axes differ in the reset of f."""
    for src in range(1, 41):
        for dst in range(1, 41):
            assert_tables(rip_lib, 7, src, 5, dst)
            assert_tables(rip_lib, src, 9, dst, 4)


@pytest.mark.parametrize("src,dst", LARGE_PAIRS)
def test_host_tables_equal_the_reference_for_large_sides(rip_lib, src, dst):
    assert_tables(rip_lib, 11, src, 7, dst)
    assert_tables(rip_lib, src, 11, dst, 7)
    assert_tables(rip_lib, src, src, dst, dst)


def test_table_properties(rip_lib):
    """What the kernel relies on: taps inside the image, weights of 11 bits, the flag only for 2 x on both axes."""
    for (R_, C_, H, W) in ((5, 611, 9, 1027), (23, 1747, 1, 1027), (10, 2050, 5, 1025), (10, 2050, 7, 1025), (1, 1, 40, 40), (16384, 3, 3, 16384)):
        st, t = hook(rip_lib, R_, C_, H, W)
        assert st == P.RIP_OK
        assert t["xofs"].min() >= 0 and t["xofs"].max() <= C_ - 1 and t["yofs"].min() >= 0 and t["yofs"].max() <= R_ - 1
        for w in (t["alpha"], t["beta"]):
            assert w.min() >= 0 and w.max() <= 2048
        assert (t["alpha"][t["xofs"] == C_ - 1, 1] == 0).all()      # no second tap beyond the last column
        assert t["area2"] == int(R_ == 2 * H and C_ == 2 * W)


def test_the_hook_refuses_bad_sizes_and_null_tables(rip_lib):
    a32, a16 = np.full(8, -7, np.int32), np.full(8, -7, np.int16)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for bad in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (-1, 4, 4, 4), (16385, 4, 4, 4), (4, 4, 4, 16385)):
        assert rip_lib.rip_debug_resize_tables(*bad, ptr(a32), ptr(a16), ptr(a32), ptr(a16), None) == INVALID, bad
        assert (a32 == -7).all() and (a16 == -7).all()
    assert rip_lib.rip_debug_resize_tables(4, 4, 4, 4, None, ptr(a16), ptr(a32), ptr(a16), None) == INVALID


# ---- the reference against the oracle -----------------------------------------------------------------------------------------
def pairs_for_images():
    out = [(6, 10, 3, 5), (6, 10, 3, 4), (6, 12, 3, 4), (6, 10, 2, 5), (5, 7, 5, 7), (1, 1, 1, 1), (1, 1, 7, 9), (7, 9, 1, 1), (9, 1747, 5, 1027), (5, 611, 9, 1027),
           (10, 2050, 5, 1025), (10, 2050, 4, 1025), (23, 13, 40, 3), (3, 40, 17, 41)]
    rng = np.random.default_rng(31)
    out += [tuple(int(v) for v in rng.integers(1, 61, 4)) for _ in range(60)]
    return out


def test_the_reference_equals_the_oracle(oracle):
    """Both channel counts; (2H, 2W) takes the 2 x 2 mean, (2H, 3W) and (3H, 2W)-like pairs stay linear, identity sizes are the identity."""
    rng = np.random.default_rng(5)
    for (R_, C_, H, W) in pairs_for_images():
        for cn in (1, 3):
            f = rng.integers(0, 256, (R_, C_) if cn == 1 else (R_, C_, 3), dtype=np.uint8)
            want = oracle.resize_linear(f, H, W)
            got = Z.resize(f, H, W)
            assert got.shape == want.shape and np.array_equal(got, want), "%d x %d x %d -> %d x %d" % (R_, C_, cn, H, W)
            if (R_, C_) == (H, W):
                assert np.array_equal(got, f)


def test_known_answers():
    f = np.array([[0, 100], [200, 255]], np.uint8)
    assert Z.resize(f, 1, 1).tolist() == [[(0 + 100 + 200 + 255 + 2) >> 2]]          # the 2 x 2 mean
    up = Z.resize(np.array([[0, 255]], np.uint8), 1, 4)                               # f = -0.25 (clamped), 0.25, 0.75, 1.25 (clamped)
    assert up.tolist() == [[0, 64, 191, 255]]
    t = Z.tables(4, 4, 2, 3)                                                          # 2 x on y only: not the mean
    assert t["area2"] == 0 and t["yofs"].tolist() == [[0, 1], [2, 3]] and t["beta"].tolist() == [[1024, 1024], [1024, 1024]]
    assert Z.tables(3, 3, 6, 3)["yofs"][0].tolist() == [0, 0]                         # sy = -1: both rows clamp to row 0


# ---- the parameter surface -------------------------------------------------------------------------------------------------
def test_defaults_set_get_and_reject(host_pipe):
    p = host_pipe
    assert p.get_output_size() == (0, 0)
    for size in ((640, 512), (1, 1), (16384, 16384), (1, 16384), (0, 0), (7, 3)):
        p.set_output_size(*size)
        assert p.get_output_size() == size
    for bad in ((0, 3), (7, 0), (-1, 3), (7, -3), (-1, -1), (16385, 3), (7, 16385), (1 << 30, 1 << 30)):
        with pytest.raises(ValueError) as e:
            p.set_output_size(*bad)
        assert "16384" in str(e.value) and "(0, 0)" in str(e.value)
        assert p.get_output_size() == (7, 3)
    lib = p._lib
    assert lib.rip_set_output_size(None, 4, 4) == INVALID and lib.rip_get_output_size(None, None, None) == INVALID
    assert lib.rip_get_output_size(p._h, None, None) == P.RIP_OK


def write_params(tmp_path, text):
    path = tmp_path / "params.yaml"
    path.write_text(text)
    return str(path)


def test_yaml_key(tmp_path, host_pipe):
    p = host_pipe
    p.load_params(write_params(tmp_path, "output:\n  size: [640, 512]\n  format: rgb8\n"))
    assert p.get_output_size() == (640, 512) and p.get_output_format() == "rgb8"
    p.load_params(write_params(tmp_path, "output:\n  format: mono8\n"))            # absent: off
    assert p.get_output_size() == (0, 0)
    p.set_output_size(9, 9)
    p.load_params(write_params(tmp_path, "output:\n  size: [0, 0]\n"))
    assert p.get_output_size() == (0, 0)
    p.set_output_size(9, 9)
    p.load_params(write_params(tmp_path, "debayer:\n  enabled: true\n"))           # rip_load_params re-creates the modules
    assert p.get_output_size() == (0, 0)


@pytest.mark.parametrize("bad", ["[640]", "[640, 512, 3]", "[0, 512]", "[640, 0]", "[-1, -1]", "[16385, 4]", "[640.5, 512]", "640", "[a, 4]"])
def test_yaml_invalid_value_fails_and_changes_nothing(tmp_path, host_pipe, bad):
    p = host_pipe
    p.set_output_size(33, 17)
    p.set_output_format("bgr_chw_f32")
    p.set_flip(True)
    p.set_flip_angle(180)
    with pytest.raises((ValueError, P.RipIOError)) as e:
        p.load_params(write_params(tmp_path, "output:\n  size: %s\n  format: rgb8\nflip:\n  enabled: false\n  angle: 90\n" % bad))
    if bad != "[a, 4]":      # a word where a number belongs is the YAML reader's own kind of failure
        assert isinstance(e.value, ValueError), e.value
    assert p.get_output_size() == (33, 17) and p.get_output_format() == "bgr_chw_f32" and p.is_flip_enabled()


# ---- geometry ------------------------------------------------------------------------------------------------------------
def expect_geometry(p, rows, cols, cn, enc, fmt, out_rows, out_cols, native_channels=3):
    if fmt == "native":
        planes, elem, planar, name = native_channels, 1, False, ("bgr8" if native_channels == 3 else "mono8")
        if enc == "rgb8":
            name = "rgb8"
    else:
        planes, elem, planar, name = (1 if fmt == "mono8" else 3), R.ELEM_BYTES[fmt], R.is_planar(fmt), fmt
    assert p.query_output(rows, cols, cn, enc) == (out_rows, out_cols, planes, name), (fmt, enc)
    assert p.query_output_bytes(rows, cols, cn, enc) == (out_rows * out_cols * planes * elem, elem, planar), (fmt, enc)


def neutral(p):
    for setter in ("set_white_balance", "set_undistortion", "set_vignetting_correction", "set_color_calibration", "set_gamma_correction",
                   "set_color_enhancer", "set_flip"):
        getattr(p, setter)(False)


def test_geometry_per_format_with_and_without_a_target(host_pipe):
    p = host_pipe
    neutral(p)
    for fmt in ("native",) + R.FORMATS:
        p.set_output_format(fmt)
        for target, (orows, ocols) in (((0, 0), (30, 44)), ((44, 30), (30, 44)), ((17, 9), (9, 17)), ((88, 60), (60, 88)), ((22, 15), (15, 22))):
            p.set_output_size(*target)
            p.set_flip(False)
            for cn, enc in ((1, "bayer_rggb8"), (3, "bgr8"), (3, "rgb8"), (1, "bayer_gbrg12p")):
                expect_geometry(p, 30, 44, cn, enc, fmt, orows, ocols)
            assert p.query_taps(30, 44, 1, "bayer_rggb8") == (30, 44, 3)          # the taps do not depend on the target
        p.set_output_size(17, 9)
        p.set_flip(True)
        p.set_flip_angle(90)
        expect_geometry(p, 30, 44, 1, "bayer_rggb8", fmt, 9, 17)
        assert p.query_taps(30, 44, 1, "bayer_rggb8") == (44, 30, 3)


def test_geometry_of_mono_frames_and_the_format_rules(host_pipe):
    p = host_pipe
    neutral(p)
    p.set_output_size(17, 9)
    for fmt in ("native", "mono8"):
        p.set_output_format(fmt)
        expect_geometry(p, 30, 44, 1, "mono8", fmt, 9, 17, native_channels=1)
    for fmt in R.FORMATS:
        if fmt == "mono8":
            continue
        p.set_output_format(fmt)
        with pytest.raises(ValueError):                                             # unchanged: a one-channel result takes mono8 or native
            p.query_output(30, 44, 1, "mono8")
    assert p.query_taps(30, 44, 1, "mono8") == (30, 44, 1)


def test_geometry_with_a_new_undistortion_image_size(host_pipe):
    p = host_pipe
    neutral(p)
    synth.load_camera(p, synth.camera_model(64, 48))
    p.set_undistortion(True)
    p.set_undistortion_new_image_size(40, 24)
    rows, cols = p.get_dist_image_height(), p.get_dist_image_width()
    for fmt in ("native",) + R.FORMATS:
        p.set_output_format(fmt)
        p.set_output_size(0, 0)
        expect_geometry(p, 48, 64, 1, "bayer_bggr8", fmt, rows, cols)
        p.set_output_size(cols, rows)                                               # the target is F's size
        expect_geometry(p, 48, 64, 1, "bayer_bggr8", fmt, rows, cols)
        p.set_output_size(21, 13)
        expect_geometry(p, 48, 64, 1, "bayer_bggr8", fmt, 13, 21)


def test_refusals(host_pipe):
    p = host_pipe
    neutral(p)
    p.set_debayer_16bit(True)
    for target in ((17, 9), (44, 30)):                                              # a target on a bgr16 result, F's own size included
        p.set_output_size(*target)
        for call in (p.query_output, p.query_output_bytes, p.get_output_camera_info):
            with pytest.raises(ValueError) as e:
                call(30, 44, 1, "bayer_rggb16")
            assert "bgr16" in str(e.value)
    p.set_debayer_16bit_range(64, 1023)                                             # with a range the frame is an 8-bit one
    p.set_output_size(17, 9)
    expect_geometry(p, 30, 44, 1, "bayer_rggb16", "native", 9, 17)
    p.set_debayer_16bit_range(0, 0)
    p.set_output_size(0, 0)
    assert p.query_output(30, 44, 1, "bayer_rggb16") == (30, 44, 3, "bgr16")
    p.set_output_size(64, 64)                                                       # an F larger than 16384 on a side
    for rows, cols in ((8, 16385), (16385, 8)):
        with pytest.raises(ValueError) as e:
            p.query_output(rows, cols, 1, "mono8")
        assert "16384" in str(e.value)
    assert p.query_output(8, 16384, 1, "mono8") == (64, 64, 1, "mono8")
    p.set_output_size(0, 0)
    assert p.query_output(8, 16385, 1, "mono8") == (8, 16385, 1, "mono8")           # without a target every size is what it was


def test_frame_calls_need_a_device_under_a_target_too(host_pipe):
    host_pipe.set_output_size(4, 4)
    with pytest.raises(P.RipError):
        host_pipe.process(np.zeros((8, 8), np.uint8), "bayer_rggb8")


# ---- the camera matrix of the delivered image -------------------------------------------------------------------------------
def test_camera_info_equals_the_scaled_matrices(host_pipe):
    p = host_pipe
    neutral(p)
    cam = synth.camera_model(64, 48)
    synth.load_camera(p, cam)
    for undistort, new_size in ((False, None), (True, None), (True, (40, 24))):
        p.set_undistortion(undistort)
        if new_size:
            p.set_undistortion_new_image_size(*new_size)
        k0 = p.get_rect_camera_matrix() if undistort else p.get_dist_camera_matrix()
        p0 = p.get_rect_projection_matrix() if undistort else p.get_dist_projection_matrix()
        rows, cols = (p.get_dist_image_height(), p.get_dist_image_width()) if undistort else (48, 64)
        assert np.count_nonzero(k0) >= 5
        p.set_output_size(0, 0)
        h, w, k, pr = p.get_output_camera_info(48, 64, 1, "bayer_rggb8")
        assert (h, w) == (rows, cols) and np.array_equal(k, k0) and np.array_equal(pr, p0)
        for target in ((cols, rows), (21, 13), (640, 512), (cols // 2, rows // 2), (1, 1), (16384, 3)):
            p.set_output_size(*target)
            h, w, k, pr = p.get_output_camera_info(48, 64, 1, "bayer_rggb8")
            wk, wp = Z.scaled_camera(k0, p0, rows, cols, target[1], target[0])
            assert (h, w) == (target[1], target[0])
            assert np.array_equal(k, wk) and np.array_equal(pr, wp), (undistort, target)
            if target == (cols, rows):
                assert np.array_equal(k, k0) and np.array_equal(pr, p0)
    # a flip by 90 degrees swaps the sides of F the factors are taken from
    p.set_undistortion(False)
    p.set_flip(True)
    p.set_flip_angle(90)
    p.set_output_size(24, 128)
    h, w, k, _ = p.get_output_camera_info(48, 64, 1, "bayer_rggb8")
    assert (h, w) == (128, 24) and np.array_equal(k, Z.scaled_camera(p.get_dist_camera_matrix(), p.get_dist_projection_matrix(), 64, 48, 128, 24)[0])
    assert p._lib.rip_get_output_camera_info(p._h, 48, 64, 1, b"bayer_rggb8", None, None, None, None) == P.RIP_OK
    assert p._lib.rip_get_output_camera_info(p._h, 48, 64, 1, None, None, None, None, None) == INVALID


def test_scaled_camera_maps_pixel_centres():
    """A point at source position u lands at a (u + 0.5) - 0.5: the corners of the image stay the corners."""
    k = np.array([[100.0, 0, 31.5], [0, 90.0, 23.5], [0, 0, 1]])
    pm = np.hstack([k, [[5.0], [7.0], [0.0]]])
    k2, p2 = Z.scaled_camera(k, pm, 48, 64, 24, 32)
    assert k2.tolist() == [[50.0, 0, 15.5], [0, 45.0, 11.5], [0, 0, 1]] and p2[:, 3].tolist() == [2.5, 3.5, 0.0]
    x = np.array([0.2, -0.1, 1.0])
    u, u2 = (k @ x)[:2], (k2 @ x)[:2]
    assert np.allclose(u2, 0.5 * (u + 0.5) - 0.5)


# ---- C++ facade ------------------------------------------------------------------------------------------------------------
def build_resize_test(tmp_path, branch):
    exe = str(tmp_path / ("resize_test_" + branch.replace("-", "_")))
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror"] + BRANCHES[branch] + ["-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "resize_test.cpp"), "-o", exe, "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir,
           "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade_sets_gets_and_throws(tmp_path, rip_lib, branch):
    exe = build_resize_test(tmp_path, branch)
    r = subprocess.run([exe, "host"], capture_output=True, text=True, env=run_env(-1))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "resize host OK" in r.stdout and "no CPU execution path" in r.stdout


# ---- the kernel, executed on the host ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_kernel_run_on_the_host_equals_the_oracle_byte_for_byte(tmp_path, rip_lib, oracle, sanitize):
    """tests/cpp/resize_kernel_host.cpp: csrc/rip_resize.hip compiled as host code, every thread of the launcher's grid run in turn,
    both channel counts x the widths around the lane and the workgroup x down- / upscale / the 2 x 2 path x pitches, offsets and
    frame gaps, plus 3000 seeded cases; exactly sized buffers with sentinels.  The second build adds -fsanitize=address,undefined
    to this stand-alone program (no out-of-bounds access, no misaligned wide access)."""
    obj = str(tmp_path / "rip_oracle.o")
    cc = os.path.join(os.path.dirname(host_clangxx()), "clang")
    r = subprocess.run([cc, "-O1", "-c", "-x", "c"] + (HOST_SANITIZE if sanitize else []) + [os.path.join(ROOT, "oracle", "rip_oracle.c"), "-I", os.path.join(ROOT, "oracle"), "-o", obj],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = build_host_program(tmp_path, "resize_kernel_host", ["resize_kernel_host.cpp", os.path.join(CSRC, "rip_output_tables.cpp")], sanitize=sanitize,
                             extra=["-ffp-contract=off", obj, "-lm", "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "3376 cases, 0 bad" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
