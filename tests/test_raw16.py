"""The 16-bit range (rip_set_debayer_16bit_range) without a GPU: the narrowing's known answers, the parameter surface on
RIP_DEVICE_NONE handles, geometry queries, the params YAML keys, the front-end parameters, the C++ facade, and what the
compiler made of rip_raw16.hip (no scratch, no spills, no hazards)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import raw16_cases as G
from helpers import LAYOUTS
from raw16_reference import narrow16
from raw_image_pipeline_amd import RipAssertError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the narrowing ------------------------------------------------------------------------------------------------------------
def n1(v, black, white):
    return int(narrow16(np.array([v]), black, white)[0])


def test_known_answers_of_the_formula():
    assert n1(128, 0, 65535) == 0 and n1(129, 0, 65535) == 1 and n1(65535, 0, 65535) == 255
    assert np.array_equal(narrow16(np.arange(256), 0, 255), np.arange(256))
    assert np.array_equal(narrow16(256 * np.arange(256), 0, 65280), np.arange(256))
    assert not narrow16(np.arange(65), 64, 1023).any() and n1(1023, 64, 1023) == 255
    assert n1(65535, 64, 1023) == 255 and n1(1022, 64, 1023) == 255 and n1(1021, 64, 1023) == 254
    assert n1(0, 0, 1) == 0 and n1(1, 0, 1) == 255 and n1(65534, 65534, 65535) == 0 and n1(65535, 65534, 65535) == 255
    # rounded half up: 255 * v / 510 = v / 2
    assert n1(1, 0, 510) == 1 and n1(2, 0, 510) == 1 and n1(3, 0, 510) == 2
    # the numerator stays below 2^26
    assert 510 * 65535 + 65535 < 1 << 26


def lib_narrow(rip_lib, values, black, white):
    v = np.ascontiguousarray(values, np.uint16)
    out = np.empty(v.size, np.uint8)
    rip_lib.rip_debug_raw16_narrow.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    st = rip_lib.rip_debug_raw16_narrow(black, white, v.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_size_t(v.size))
    assert st == 0, (black, white)
    return out


def test_the_kernels_multiplier_equals_the_division_for_every_value(rip_lib):
    """The launch constants of rip_raw16.hip (a multiplier and a shift instead of the division by 2 R), through the host
    restatement of the kernel's arithmetic: all 65536 values for the ranges of the GPU test, the edge ranges and 300 random ones."""
    rng = np.random.default_rng(16)
    ranges = list(G.RANGES) + [(0, 2), (0, 3), (65533, 65535), (0, 32767), (0, 32768), (0, 32769), (1, 65535), (0, 65534), (32767, 32768)]
    ranges += [(2 ** k - 1, 2 ** k) for k in range(1, 16)] + [(0, 2 ** k) for k in range(1, 16)] + [(0, 2 ** k + 1) for k in range(1, 15)]
    for _ in range(300):
        ranges.append(G.random_range(rng))
    values = np.arange(65536)
    for black, white in ranges:
        got, want = lib_narrow(rip_lib, values, black, white), narrow16(values, black, white)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "(%d, %d): n(%d) = %d, expected %d" % (black, white, bad[0], got[bad[0]], want[bad[0]])


def test_the_hook_rejects_what_the_setter_rejects(rip_lib):
    rip_lib.rip_debug_raw16_narrow.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    for black, white in ((0, 0), (-1, 5), (5, 5), (0, 65536)):
        assert rip_lib.rip_debug_raw16_narrow(black, white, None, None, C.c_size_t(0)) == 1


# ---- parameter surface on RIP_DEVICE_NONE handles ---------------------------------------------------------------------------------
INVALID = [(-1, 100), (0, 65536), (500, 500), (600, 500), (5, 0), (-5, -1), (65535, 65535), (70000, 80000)]


def test_default_set_get_and_reject(host_pipe):
    assert host_pipe.get_debayer_16bit_range() == (0, 0)
    host_pipe.set_debayer_16bit_range(64, 1023)
    assert host_pipe.get_debayer_16bit_range() == (64, 1023)
    for black, white in INVALID:
        with pytest.raises(ValueError):
            host_pipe.set_debayer_16bit_range(black, white)
        assert host_pipe.get_debayer_16bit_range() == (64, 1023)
    for black, white in ((0, 65535), (0, 1), (65534, 65535), (0, 0)):
        host_pipe.set_debayer_16bit_range(black, white)
        assert host_pipe.get_debayer_16bit_range() == (black, white)


def test_null_pointers_of_the_getter(rip_lib, host_pipe):
    host_pipe.set_debayer_16bit_range(3, 9)
    w = C.c_int()
    assert rip_lib.rip_get_debayer_16bit_range(host_pipe._h, None, C.byref(w)) == 0 and w.value == 9
    assert rip_lib.rip_get_debayer_16bit_range(host_pipe._h, None, None) == 0


def everything_on(p, angle=0):
    p.set_flip(angle != 0)
    p.set_flip_angle(angle)
    p.set_white_balance(True)
    p.set_white_balance_method("simple")
    p.set_color_calibration(True)
    p.set_gamma_correction(True)
    p.set_vignetting_correction(True)
    p.set_color_enhancer(True)


def test_a_rejected_call_changes_nothing(host_pipe):
    host_pipe.set_debayer_16bit(True)
    host_pipe.set_debayer_16bit_range(64, 1023)
    everything_on(host_pipe, 90)
    before = (host_pipe.query_output(48, 64, 1, "bayer_rggb16"), host_pipe.query_taps(48, 64, 1, "bayer_rggb16"))
    for black, white in INVALID:
        with pytest.raises(ValueError):
            host_pipe.set_debayer_16bit_range(black, white)
    assert (host_pipe.query_output(48, 64, 1, "bayer_rggb16"), host_pipe.query_taps(48, 64, 1, "bayer_rggb16")) == before


@pytest.mark.parametrize("method", G.METHODS)
@pytest.mark.parametrize("name", G.NAMES)
def test_query_output_and_taps_with_every_stage_on(host_pipe, name, method):
    p = host_pipe
    p.set_debayer_16bit(True)
    p.set_debayer_16bit_range(64, 1023)
    p.set_debayer_method(method)
    enc = G.enc16(name)
    for angle in (0, 180):
        everything_on(p, angle)
        assert p.query_output(48, 64, 1, enc) == (48, 64, 3, "bgr8")
        assert p.query_taps(48, 64, 1, enc) == (48, 64, 3)
    for angle in (90, 270):
        everything_on(p, angle)
        assert p.query_output(48, 64, 1, enc) == (64, 48, 3, "bgr8")
        assert p.query_taps(48, 64, 1, enc) == (64, 48, 3)
    # undistortion: the output takes the calibration's size, the taps keep the post-flip one
    from raw_image_pipeline_amd import synth
    everything_on(p, 90)
    synth.load_camera(p, synth.camera_model(48, 64))
    p.set_undistortion(True)
    assert p.query_output(48, 64, 1, enc) == (64, 48, 3, "bgr8")
    assert p.query_taps(48, 64, 1, enc) == (64, 48, 3)
    # the checks of the 8-bit Bayer path still hold
    with pytest.raises(RipAssertError):
        p.query_output(48, 64, 3, enc)
    with pytest.raises(RipAssertError):
        p.query_output(2, 64, 1, enc)


def test_a_range_without_the_opt_in_has_no_effect(host_pipe):
    host_pipe.set_debayer_16bit_range(64, 1023)
    with pytest.raises(ValueError, match="valid pattern but is not supported"):
        host_pipe.query_output(48, 64, 1, "bayer_gbrg16")
    assert host_pipe.query_output(48, 64, 1, "bayer_gbrg8") == (48, 64, 3, "bgr8")


def test_with_the_range_back_at_zero_the_handle_answers_as_before(host_pipe):
    p = host_pipe
    p.set_white_balance(False)
    p.set_undistortion(False)
    p.set_debayer_16bit(True)
    assert p.query_output(48, 64, 1, "bayer_gbrg16") == (48, 64, 3, "bgr16")
    p.set_debayer_16bit_range(0, 4095)
    assert p.query_output(48, 64, 1, "bayer_gbrg16") == (48, 64, 3, "bgr8")
    p.set_gamma_correction(True)
    assert p.query_output(48, 64, 1, "bayer_gbrg16") == (48, 64, 3, "bgr8")
    p.set_debayer_16bit_range(0, 0)
    with pytest.raises(RipAssertError):   # 8-bit stages and a bgr16 result
        p.query_output(48, 64, 1, "bayer_gbrg16")
    p.set_gamma_correction(False)
    p.set_flip(True)
    p.set_flip_angle(270)
    assert p.query_output(48, 64, 1, "bayer_gbrg16") == (64, 48, 3, "bgr16")
    # 8-bit encodings never see the setting
    p.set_debayer_16bit_range(10, 20)
    assert p.query_output(48, 64, 1, "bayer_gbrg8") == (64, 48, 3, "bgr8")
    assert p.query_output(48, 64, 1, "mono8") == (64, 48, 1, "mono8")


def test_dtype_and_encoding_must_agree(host_pipe):
    host_pipe.set_debayer_16bit(True)
    host_pipe.set_debayer_16bit_range(0, 1023)
    with pytest.raises(ValueError, match="does not match"):
        host_pipe.process(np.zeros((8, 8), np.uint8), "bayer_rggb16")
    with pytest.raises(ValueError, match="does not match"):
        host_pipe.process(np.zeros((8, 8), np.uint16), "bayer_rggb8")
    with pytest.raises(ValueError, match="does not match"):
        host_pipe.submit(np.zeros((8, 8), np.uint8), "bayer_rggb16")


# ---- params YAML ------------------------------------------------------------------------------------------------------------------
def write_params(tmp_path, text):
    path = tmp_path / "params.yaml"
    path.write_text(text)
    return str(path)


def test_yaml_keys(tmp_path, host_pipe):
    p = host_pipe
    p.load_params(write_params(tmp_path, "debayer:\n  enabled: true\n  accept_16bit: true\n  black_level: 64\n  white_level: 1023\ngamma_correction:\n  enabled: true\n"))
    assert p.get_debayer_16bit_range() == (64, 1023)
    assert p.query_output(20, 30, 1, "bayer_rggb16") == (20, 30, 3, "bgr8")
    # the levels without accept_16bit: stored, without effect
    p.load_params(write_params(tmp_path, "debayer:\n  black_level: 0\n  white_level: 4095\n"))
    assert p.get_debayer_16bit_range() == (0, 4095)
    with pytest.raises(ValueError, match="valid pattern but is not supported"):
        p.query_output(20, 30, 1, "bayer_rggb16")
    # accept_16bit alone: today's bgr16
    p.load_params(write_params(tmp_path, "debayer:\n  accept_16bit: true\n"))
    assert p.get_debayer_16bit_range() == (0, 0)
    assert p.query_output(20, 30, 1, "bayer_rggb16") == (20, 30, 3, "bgr16")
    # a file without the keys re-creates the module with the defaults, as loadParams does for every key
    p.set_debayer_16bit_range(1, 2)
    p.load_params(write_params(tmp_path, "debayer:\n  enabled: true\n"))
    assert p.get_debayer_16bit_range() == (0, 0)
    with pytest.raises(ValueError, match="valid pattern but is not supported"):
        p.query_output(20, 30, 1, "bayer_rggb16")


@pytest.mark.parametrize("levels", ["black_level: 1023\n  white_level: 64", "black_level: -1\n  white_level: 64", "white_level: 65536",
                                    "black_level: 7\n  white_level: 7", "black_level: 7"])
def test_yaml_invalid_range_fails_and_changes_nothing(tmp_path, host_pipe, levels):
    p = host_pipe
    p.set_debayer_16bit(True)
    p.set_debayer_16bit_range(64, 1023)
    p.set_debayer_method("mht")
    p.set_flip(True)
    p.set_flip_angle(180)
    p.set_gamma_correction(True)
    before = p.query_output(20, 30, 1, "bayer_rggb16")
    with pytest.raises(ValueError, match="0 <= black < white <= 65535"):
        p.load_params(write_params(tmp_path, "debayer:\n  accept_16bit: false\n  method: bilinear\n  %s\nflip:\n  enabled: false\n  angle: 90\n" % levels))
    assert p.get_debayer_16bit_range() == (64, 1023) and p.get_debayer_method() == "mht"
    assert p.is_flip_enabled() and p.is_gamma_correction_enabled()
    assert p.query_output(20, 30, 1, "bayer_rggb16") == before == (20, 30, 3, "bgr8")


# ---- front end ------------------------------------------------------------------------------------------------------------------
def test_frontend_parameters_map_to_the_handle(rip_lib):
    from raw_image_pipeline_amd import RawImagePipeline
    from raw_image_pipeline_amd.frontend import NODE_DEFAULTS, CameraStream
    assert NODE_DEFAULTS["debayer/accept_16bit"] is False and NODE_DEFAULTS["debayer/black_level"] == 0 and NODE_DEFAULTS["debayer/white_level"] == 0
    cam = CameraStream({}, pipeline=RawImagePipeline(False, device=-1))
    assert cam.pipe.get_debayer_16bit_range() == (0, 0)
    with pytest.raises(ValueError, match="valid pattern but is not supported"):
        cam.pipe.query_output(20, 30, 1, "bayer_rggb16")
    cam = CameraStream({"debayer/accept_16bit": True, "debayer/black_level": 256, "debayer/white_level": 4095, "gamma_correction/enabled": True},
                       pipeline=RawImagePipeline(False, device=-1))
    assert cam.pipe.get_debayer_16bit_range() == (256, 4095)
    assert cam.pipe.query_output(20, 30, 1, "bayer_rggb16") == (20, 30, 3, "bgr8")
    with pytest.raises(ValueError):
        CameraStream({"debayer/accept_16bit": True, "debayer/black_level": 4095, "debayer/white_level": 256}, pipeline=RawImagePipeline(False, device=-1))


# ---- the fuzz generator of tests/test_raw16_gpu.py ------------------------------------------------------------------------------
def test_fuzz_generator_only_produces_valid_cases(host_pipe):
    """Every generated case is one the library accepts and the GPU test compares: geometry queries succeed under its
    configuration, the range is valid, and the default count reaches both methods, every pattern, flip and layout, batches of
    several frame groups, taps given and not given, and data outside the range."""
    from helpers import configure
    cases = [G.fuzz_case(s) for s in range(G.N_FUZZ)]
    assert len(cases) == G.N_FUZZ >= 40
    for case in cases:
        assert 0 <= case["black"] < case["white"] <= 65535, case
        assert case["w"] >= 3 and case["h"] >= 3 and case["n"] >= 1
        configure(host_pipe, dict(case["c"], cam=None))   # the camera needs no device either, but loading 40 of them takes long
        host_pipe.set_debayer_method(case["method"])
        host_pipe.set_debayer_16bit(True)
        host_pipe.set_debayer_16bit_range(case["black"], case["white"])
        ow, oh = (case["h"], case["w"]) if case["flip"] in (90, 270) else (case["w"], case["h"])
        assert host_pipe.query_taps(case["h"], case["w"], 1, G.enc16(case["name"])) == (oh, ow, 3)
        frame = G.gen_frame16(case["w"], case["h"], case["name"], case["seed"], case["black"], case["white"], kind=case["kind"], tint=case["tint"])
        assert frame.dtype == np.uint16 and frame.shape == (case["h"], case["w"])
    assert {c["method"] for c in cases} == set(G.METHODS) and {c["name"] for c in cases} == set(G.NAMES)
    assert {c["flip"] for c in cases} == set(G.FLIPS) and {c["layout"] for c in cases} == set(LAYOUTS)
    assert {c["tap"] for c in cases} == {False, True} and any(c["n"] >= 9 for c in cases) and any(c["n"] == 1 for c in cases)
    assert any(min(c["w"], c["h"]) < 9 for c in cases) and any(c["w"] >= 200 and c["h"] >= 100 for c in cases)


def test_frames_of_the_generator_leave_the_range_on_both_sides():
    for black, white in ((64, 1023), (0, 65535), (1000, 1001), (65534, 65535)):
        f = G.gen_frame16(64, 48, "rggb", 1, black, white)
        assert f.min() <= black and f.max() >= white


# ---- C++ facade -------------------------------------------------------------------------------------------------------------------
def build_cpp(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "raw16_test.cpp")
    exe = str(tmp_path / "raw16_test")
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-DRIP_NO_OPENCV", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
           "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_facade_sets_and_gets_the_range(tmp_path, rip_lib):
    exe = build_cpp(tmp_path)
    env = dict(os.environ)
    env["RIP_DEVICE"] = "-1"
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "raw16 range OK" in r.stdout


# ---- what the compiler made of the kernel -----------------------------------------------------------------------------------------
RAW16_SRC = os.path.join(ROOT, "raw_image_pipeline_amd", "csrc", "rip_raw16.hip")


def test_raw16_source_has_no_scratch_or_spills():
    """hipcc -Rpass-analysis=kernel-resource-usage on rip_raw16.hip: no private segment, no spilled registers."""
    from raw_image_pipeline_amd import build as B
    cmd = [B.hipcc()] + B.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-x", "hip", "-c", RAW16_SRC, "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    kernels = r.stderr.count("Function Name:")
    assert kernels == 32, r.stderr  # 2 methods x 4 patterns x 4 flips
    scratch = [l for l in r.stderr.splitlines() if "ScratchSize" in l]
    spills = [l for l in r.stderr.splitlines() if "Spill:" in l]
    assert len(scratch) == kernels and all(l.rstrip().endswith(" 0 [-Rpass-analysis=kernel-resource-usage]") for l in scratch), scratch
    assert spills and all(l.rstrip().endswith(" 0 [-Rpass-analysis=kernel-resource-usage]") for l in spills), spills
    lds = [int(l.split("LDS Size [bytes/block]:")[1].split()[0]) for l in r.stderr.splitlines() if "LDS Size" in l]
    assert len(lds) == kernels and max(lds) <= 5040 + 6144, lds   # the uint16 tile; quarter turns add the 6 KB BGR tile


def test_raw16_source_has_no_isa_hazards():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_hazard_check.py"), RAW16_SRC], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rip_raw16.hip: 0 finding(s)" in r.stdout, r.stdout


def test_raw16_source_is_compiled_into_the_library():
    from raw_image_pipeline_amd import build as B
    assert "rip_raw16.hip" in B.SOURCES
