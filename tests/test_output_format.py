"""The output stage (include/rip.h rip_set_output_format / rip_set_output_normalization) without a GPU: the host-built tables
against tests/output_reference.py bit for bit, the mono8 formula's known answers, validation, the YAML keys, the geometry
queries on RIP_DEVICE_NONE handles and the C++ facade's setters, getters and throws."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import output_reference as R
from raw_image_pipeline_amd import pipeline as P
from raw_image_pipeline_amd import synth
from test_cpp_facade import BRANCHES, run_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = P.RIP_ERR_INVALID_ARGUMENT

FIXED_NORMS = {
    "defaults": R.DEFAULT_NORM,
    "imagenet_rgb": (255.0, R.IMAGENET_MEAN_RGB, R.IMAGENET_STD_RGB),
    "imagenet_bgr": (255.0, R.IMAGENET_MEAN_RGB[::-1], R.IMAGENET_STD_RGB[::-1]),
    "raw_values": (1.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    "negative_std": (255.0, (0.5, 0.25, 0.125), (-0.25, 0.5, -2.0)),
    "f16_overflows": (255.0, (0.0, 0.0, 0.0), (1e-6, 1e-5, 1.0 / 65520.0)),   # 1 / std beyond 65504: inf in f16, finite in f32
    "f16_subnormal": (255.0, (0.0, 0.0, 0.0), (3e4, 1e6, 5e7)),                # entries below 2^-14, down to 0
    "f32_overflows": (1e-300, (0.0, 0.0, 0.0), (1e-30, 1.0, 1e300)),
}


def seeded_norms(n=200, seed=20240611):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        divisor = float(10 ** rng.uniform(-3, 3)) * float(rng.choice([-1.0, 1.0, 1.0, 1.0]))
        mean = tuple(float(v) for v in rng.uniform(-2, 2, 3))
        std = tuple(float(v) for v in 10 ** rng.uniform(-8, 8, 3) * rng.choice([-1.0, 1.0, 1.0], 3))
        yield divisor, mean, std


def hook(lib, fmt, divisor, mean, std):
    out = np.full((3, 256), 0xA5A5A5A5, np.uint32).astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[R.ELEM_BYTES.get(fmt, 4)])   # 0xA5... sentinels
    st = lib.rip_debug_output_table(fmt.encode(), C.c_double(divisor), (C.c_double * 3)(*mean), (C.c_double * 3)(*std),
                                    out.ctypes.data_as(C.c_void_p))
    return st, out


@pytest.mark.parametrize("fmt", R.TABLE_FORMATS)
def test_tables_equal_the_reference_bit_for_bit(rip_lib, fmt):
    norms = list(FIXED_NORMS.items()) + [("seeded %d" % i, nrm) for i, nrm in enumerate(seeded_norms())]
    for name, (divisor, mean, std) in norms:
        st, got = hook(rip_lib, fmt, divisor, mean, std)
        assert st == P.RIP_OK, name
        ref = R.bits(R.table(fmt, divisor, mean, std))
        assert got.dtype == ref.dtype and np.array_equal(got, ref), "%s %s: %d of 768 entries differ" % (fmt, name, int((got != ref).sum()))


def test_the_fixed_parameter_sets_reach_what_they_are_named_for():
    inf16 = R.table("rgb_chw_f16", *FIXED_NORMS["f16_overflows"])
    assert np.isinf(inf16[0, 17:]).all() and np.isfinite(inf16[0, :17]).all() and np.isfinite(R.table("rgb_chw_f32", *FIXED_NORMS["f16_overflows"])).all()
    assert np.isinf(inf16[2, 255]) and np.isfinite(inf16[2, 254])   # 65520 is the first value that rounds to inf
    sub = R.bits(R.table("rgb_chw_f16", *FIXED_NORMS["f16_subnormal"])) & 0x7FFF
    assert ((sub > 0) & (sub < 0x0400)).any() and (sub[2, 1:] == 0).any()
    assert np.isinf(R.table("bgr_chw_f32", *FIXED_NORMS["f32_overflows"])[0, 1:]).all()
    assert (R.table("rgb_chw_f32", *FIXED_NORMS["negative_std"])[0, 200:] < 0).all()
    # bf16 rounds to nearest even: 1 + 2^-8 is a tie and goes down to 1, 1 + 3 * 2^-8 goes up to 1 + 2^-6
    assert list(R.bf16_bits(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -7], np.float32))) == [0x3F80, 0x3F82, 0x3F81]


def test_formats_without_a_table_and_bad_arguments_are_refused_by_the_hook(rip_lib):
    for fmt in ("rgb8", "mono8", "native", "rgb_hwc_f32", ""):
        assert hook(rip_lib, fmt, *R.DEFAULT_NORM)[0] == INVALID, fmt
    for divisor, mean, std in [(0.0, (0, 0, 0), (1, 1, 1)), (float("nan"), (0, 0, 0), (1, 1, 1)), (255.0, (0, float("inf"), 0), (1, 1, 1)),
                               (255.0, (0, 0, 0), (1, 0.0, 1)), (255.0, (0, 0, 0), (1, 1, float("nan")))]:
        st, out = hook(rip_lib, "rgb_chw_f32", divisor, mean, std)
        assert st == INVALID and (out == 0xA5A5A5A5).all()   # nothing written


def test_mono8_known_answers():
    assert list(R.mono8(np.array([[0, 0, 255], [0, 255, 0], [255, 0, 0]], np.uint8))) == [76, 150, 29]   # R, G, B primaries
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    assert np.array_equal(R.mono8(grey), np.arange(256, dtype=np.uint8))
    assert int(R.mono8(np.array([1, 2, 3], np.uint8))) == (3735 * 1 + 19235 * 2 + 9798 * 3 + 16384) >> 15 == 2
    assert 3735 + 19235 + 9798 == 1 << 15


def test_convert_reverses_and_orders_the_planes():
    e = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    assert np.array_equal(R.convert(e, "rgb8")[..., 0], e[..., 2])
    rgb = R.convert(e, "rgb_chw_f32", 1.0)
    bgr = R.convert(e, "bgr_chw_f32", 1.0)
    assert rgb.shape == (3, 2, 3) and np.array_equal(rgb[0], e[..., 2].astype(np.float32)) and np.array_equal(bgr[0], e[..., 0].astype(np.float32))
    assert R.convert(np.stack([e, e]), "bgr_chw_f16").shape == (2, 3, 2, 3)


# ---- the parameter surface -------------------------------------------------------------------------------------------------
def state(p):
    return p.get_output_format(), p.get_output_normalization()


def test_defaults_set_get_and_reject(host_pipe):
    p = host_pipe
    assert state(p) == ("native", R.DEFAULT_NORM)
    for fmt in R.FORMATS + ("native",):
        p.set_output_format(fmt)
        assert p.get_output_format() == fmt
    p.set_output_format("bgr_chw_bf16")
    p.set_output_normalization(2.0, (0.1, 0.2, 0.3), (-1.0, 2.0, 3.0))
    before = state(p)
    assert before == ("bgr_chw_bf16", (2.0, (0.1, 0.2, 0.3), (-1.0, 2.0, 3.0)))
    with pytest.raises(ValueError) as e:
        p.set_output_format("rgb_hwc_f32")
    for fmt in R.FORMATS + ("native",):
        assert "'%s'" % fmt in str(e.value)
    for bad in [(0.0, (0, 0, 0), (1, 1, 1)), (float("inf"), (0, 0, 0), (1, 1, 1)), (255.0, (float("nan"), 0, 0), (1, 1, 1)),
                (255.0, (0, 0, 0), (0.0, 1, 1)), (255.0, (0, 0, 0), (1, 1, float("-inf")))]:
        with pytest.raises(ValueError):
            p.set_output_normalization(*bad)
        assert state(p) == before
    with pytest.raises(ValueError):
        p.set_output_normalization(255.0, (0, 0), (1, 1, 1))
    assert state(p) == before
    lib = p._lib
    assert lib.rip_set_output_format(p._h, None) == INVALID and lib.rip_set_output_normalization(p._h, C.c_double(1.0), None, None) == INVALID
    assert lib.rip_get_output_normalization(p._h, None, None, None) == P.RIP_OK
    assert state(p) == before


def write_params(tmp_path, text):
    path = tmp_path / "params.yaml"
    path.write_text(text)
    return str(path)


def test_yaml_keys(tmp_path, host_pipe):
    p = host_pipe
    p.load_params(write_params(tmp_path, "output:\n  format: rgb_chw_f16\n  divisor: 255\n  mean: [0.485, 0.456, 0.406]\n  std: [0.229, 0.224, 0.225]\n"))
    assert state(p) == ("rgb_chw_f16", (255.0, R.IMAGENET_MEAN_RGB, R.IMAGENET_STD_RGB))
    p.load_params(write_params(tmp_path, "output:\n  format: mono8\n"))        # absent keys: the defaults
    assert state(p) == ("mono8", R.DEFAULT_NORM)
    p.load_params(write_params(tmp_path, "output:\n  divisor: 1.0\n"))
    assert state(p) == ("native", (1.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    p.set_output_format("rgb8")
    p.load_params(write_params(tmp_path, "debayer:\n  enabled: true\n"))       # rip_load_params re-creates the modules
    assert state(p) == ("native", R.DEFAULT_NORM)


@pytest.mark.parametrize("bad", ["format: rgb_hwc_f32", "divisor: 0", "std: [1, 0, 1]", "mean: [0, 1]", "std: [1, 2, 3, 4]", "divisor: .inf\n  std: [1, 1, 1]",
                                 "mean: [0, .nan, 0]"])
def test_yaml_invalid_value_fails_and_changes_nothing(tmp_path, host_pipe, bad):
    p = host_pipe
    p.set_output_format("bgr_chw_f32")
    p.set_output_normalization(2.0, (0.1, 0.2, 0.3), (1.0, 2.0, 3.0))
    p.set_flip(True)
    p.set_flip_angle(180)
    before = state(p)
    try:
        p.load_params(write_params(tmp_path, "output:\n  %s\nflip:\n  enabled: false\n  angle: 90\n" % bad))
        raised = None
    except (ValueError, P.RipIOError) as e:   # a number the YAML reader cannot parse is its own kind of failure
        raised = e
    if raised is None:   # ".inf" / ".nan" are not numbers to this reader: the key is then absent, which is valid
        assert bad.startswith(("divisor: .inf", "mean: [0, .nan")), bad
        return
    if not bad.startswith("mean: [0, .nan"):
        assert isinstance(raised, ValueError), raised
    assert state(p) == before and p.is_flip_enabled()


# ---- geometry ------------------------------------------------------------------------------------------------------------
def expect_geometry(p, rows, cols, cn, enc, fmt, out_rows, out_cols):
    planes = 1 if fmt == "mono8" else 3
    elem = R.ELEM_BYTES[fmt]
    assert p.query_output(rows, cols, cn, enc) == (out_rows, out_cols, planes, fmt), fmt
    assert p.query_output_bytes(rows, cols, cn, enc) == (out_rows * out_cols * planes * elem, elem, R.is_planar(fmt)), fmt


def test_geometry_per_format(host_pipe):
    p = host_pipe
    p.set_white_balance(False)
    p.set_undistortion(False)
    assert p.query_output_bytes(30, 44, 1, "bayer_rggb8") == (30 * 44 * 3, 1, False)       # native
    assert p.query_output_bytes(30, 44, 1, "mono8") == (30 * 44, 1, False)
    for fmt in R.FORMATS:
        p.set_output_format(fmt)
        p.set_flip(False)
        expect_geometry(p, 30, 44, 1, "bayer_rggb8", fmt, 30, 44)
        expect_geometry(p, 30, 44, 3, "bgr8", fmt, 30, 44)
        expect_geometry(p, 30, 44, 3, "rgb8", fmt, 30, 44)
        expect_geometry(p, 30, 44, 1, "bayer_gbrg12p", fmt, 30, 44)
        p.set_flip(True)
        p.set_flip_angle(90)
        expect_geometry(p, 30, 44, 1, "bayer_rggb8", fmt, 44, 30)
        assert p.query_taps(30, 44, 1, "bayer_rggb8") == (44, 30, 3)                       # the taps do not depend on the format


def test_geometry_with_a_new_undistortion_image_size(host_pipe):
    p = host_pipe
    p.set_white_balance(False)
    p.set_flip(False)
    synth.load_camera(p, synth.camera_model(64, 48))
    p.set_undistortion(True)
    p.set_undistortion_new_image_size(40, 24)
    for fmt in R.FORMATS:
        p.set_output_format(fmt)
        rows, cols = p.get_dist_image_height(), p.get_dist_image_width()
        expect_geometry(p, 48, 64, 1, "bayer_bggr8", fmt, rows, cols)


def test_refusals_and_the_mono8_identity(host_pipe):
    p = host_pipe
    p.set_white_balance(False)
    p.set_undistortion(False)
    p.set_vignetting_correction(False)
    p.set_color_calibration(False)
    p.set_gamma_correction(False)
    p.set_color_enhancer(False)
    p.set_flip(False)
    p.set_debayer_16bit(True)
    for fmt in R.FORMATS:
        p.set_output_format(fmt)
        with pytest.raises(ValueError):                 # bgr16 result
            p.query_output(30, 44, 1, "bayer_rggb16")
        with pytest.raises(ValueError):
            p.query_output_bytes(30, 44, 1, "bayer_rggb16")
        if fmt == "mono8":                              # the identity on a one-channel result
            assert p.query_output(30, 44, 1, "mono8") == (30, 44, 1, "mono8")
            assert p.query_output_bytes(30, 44, 1, "mono8") == (30 * 44, 1, False)
        else:
            with pytest.raises(ValueError):
                p.query_output(30, 44, 1, "mono8")
            with pytest.raises(ValueError):
                p.query_output_bytes(30, 44, 1, "mono8")
        assert p.query_taps(30, 44, 1, "mono8") == (30, 44, 1)
    p.set_debayer_16bit_range(64, 1023)                 # with a range the frame is an 8-bit one
    p.set_output_format("rgb_chw_f32")
    expect_geometry(p, 30, 44, 1, "bayer_rggb16", "rgb_chw_f32", 30, 44)
    p.set_output_format("native")
    p.set_debayer_16bit_range(0, 0)
    assert p.query_output(30, 44, 1, "bayer_rggb16") == (30, 44, 3, "bgr16")
    assert p.query_output_bytes(30, 44, 1, "bayer_rggb16") == (30 * 44 * 6, 2, False)


def test_frame_calls_need_a_device_under_a_format_too(host_pipe):
    host_pipe.set_output_format("rgb8")
    with pytest.raises(P.RipError):
        host_pipe.process(np.zeros((8, 8), np.uint8), "bayer_rggb8")


# ---- C++ facade ------------------------------------------------------------------------------------------------------------
def build_output_format_test(tmp_path, branch):
    exe = str(tmp_path / ("output_format_test_" + branch.replace("-", "_")))
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror"] + BRANCHES[branch] + ["-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "output_format_test.cpp"), "-o", exe, "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir,
           "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade_sets_gets_and_throws(tmp_path, rip_lib, branch):
    exe = build_output_format_test(tmp_path, branch)
    r = subprocess.run([exe, "host"], capture_output=True, text=True, env=run_env(-1))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "output format host OK" in r.stdout and "no CPU execution path" in r.stdout
