"""The "mht" debayer method (Malvar-He-Cutler, include/rip.h rip_set_debayer_method) without a GPU: the numpy restatement of
the contract against the published filter table (impulse responses, flat colours, rounding), and the parameter surface --
C-ABI, YAML key, C++ facade, Python wrapper, node parameter -- on RIP_DEVICE_NONE handles."""
import os
import subprocess

import numpy as np
import pytest

from mht_reference import FILTERS, PHASE, mht_reference, round16
from raw_image_pipeline_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = ["bayer_rggb8", "bayer_bggr8", "bayer_gbrg8", "bayer_grbg8"]

# The table of the published filters, one row per filter: weights at the centre, (0, +-1), (+-1, 0), (0, +-2), (+-2, 0),
# (+-1, +-1); divisor 16.
TABLE = {
    "K_G": (8, 4, 4, -2, -2, 0),
    "K_row": (10, 8, 0, -2, 1, -2),
    "K_col": (10, 0, 8, 1, -2, -2),
    "K_diag": (12, 0, 0, -3, -3, 4),
}


def table_weight(name, dy, dx):
    centre, h1, v1, h2, v2, diag = TABLE[name]
    return {(0, 0): centre, (0, 1): h1, (1, 0): v1, (0, 2): h2, (2, 0): v2, (1, 1): diag}.get((abs(dy), abs(dx)), 0)


def filter_of(site, channel):
    """Which filter gives `channel` (0 B, 1 G, 2 R) at a site (dy, dx) of the Bayer phase; None: the sample itself."""
    dy, dx = site
    if (dy, dx) == (0, 0):  # R site
        return {0: "K_diag", 1: "K_G", 2: None}[channel]
    if (dy, dx) == (1, 1):  # B site
        return {0: None, 1: "K_G", 2: "K_diag"}[channel]
    if dy == 0:  # G in a red row: R left / right, B above / below
        return {0: "K_col", 1: None, 2: "K_row"}[channel]
    return {0: "K_row", 1: None, 2: "K_col"}[channel]  # G in a blue row


def test_filter_dicts_match_the_table():
    for name, k in FILTERS.items():
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                assert k.get((dy, dx), 0) == table_weight(name, dy, dx), (name, dy, dx)
        assert sum(k.values()) == 16


def impulse_frame(pattern, site, h=12, w=14):
    ry, rx = PHASE[pattern[6:10]]
    iy, ix = 6 + ((site[0] + ry) & 1), 6 + ((site[1] + rx) & 1)
    f = np.full((h, w), 128, np.uint8)
    f[iy, ix] = 144
    assert ((iy - ry) & 1, (ix - rx) & 1) == site
    return f, (iy, ix)


def impulse_expected(pattern, frame, pos):
    """128 + the table weight of the impulse seen from each pixel, channel by channel (no rounding, no clamping)."""
    ry, rx = PHASE[pattern[6:10]]
    h, w = frame.shape
    out = np.empty((h, w, 3), np.int64)
    for y in range(h):
        for x in range(w):
            site = ((y - ry) & 1, (x - rx) & 1)
            for ch in range(3):
                k = filter_of(site, ch)
                out[y, x, ch] = frame[y, x] if k is None else 128 + table_weight(k, pos[0] - y, pos[1] - x)
    return out


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("site", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_impulse_response_pins_the_filters(pattern, site):
    frame, pos = impulse_frame(pattern, site)
    got = mht_reference(frame, pattern).astype(np.int64)
    exp = impulse_expected(pattern, frame, pos)
    np.testing.assert_array_equal(got, exp)
    # every weight of every filter that reaches a pixel of another class shows up at least once
    assert (got != 128).any()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("size", [(3, 3), (4, 5), (5, 7), (64, 48)])
def test_flat_colour_mosaic_comes_back_exactly(pattern, size):
    h, w = size
    rng = np.random.default_rng(h * 100 + w)
    for bgr in [(0, 0, 0), (255, 255, 255), (10, 200, 90), tuple(int(v) for v in rng.integers(0, 256, 3))]:
        img = np.empty((h, w, 3), np.uint8)
        img[:] = bgr
        got = mht_reference(synth.mosaic(img, pattern), pattern)
        np.testing.assert_array_equal(got, img, err_msg="%s %s %s" % (pattern, size, bgr))


def test_flat_colour_16bit():
    img = np.empty((6, 9, 3), np.uint16)
    img[:] = (1000, 65535, 40000)
    mosaic = np.empty((6, 9), np.uint16)
    cell = synth.PATTERNS["bayer_grbg8"]
    for dy in range(2):
        for dx in range(2):
            mosaic[dy::2, dx::2] = img[dy::2, dx::2, cell[dy][dx]]
    np.testing.assert_array_equal(mht_reference(mosaic, "bayer_grbg16"), img)


def test_rounding_is_half_to_even():
    assert list(round16(np.array([8, 24, 40, 56, -8, 2040, 2024]), 255)) == [0, 2, 2, 4, 0, 128, 126]
    # 128 everywhere, the (0, 2) neighbour of an R site 4 higher: K_G weighs it -2, so S = 2048 - 8 = 2040 (127.5 -> 128);
    # 12 higher: S = 2048 - 24 = 2024 (126.5 -> 126)
    for delta, expect in ((4, 128), (12, 126)):
        f = np.full((8, 8), 128, np.uint8)
        f[4, 6] = 128 + delta  # rggb: (4, 4) is an R site, (4, 6) its (0, +2) neighbour
        assert int(mht_reference(f, "bayer_rggb8")[4, 4, 1]) == expect


def test_clamp_and_edges_on_a_random_frame():
    rng = np.random.default_rng(5)
    f = rng.integers(0, 256, (7, 9), dtype=np.uint8)
    got = mht_reference(f, "bayer_gbrg8")
    assert got.dtype == np.uint8 and got.shape == (7, 9, 3)
    # the sampled colour passes through unchanged
    ry, rx = PHASE["gbrg"]
    for y in range(7):
        for x in range(9):
            site = ((y - ry) & 1, (x - rx) & 1)
            ch = 2 if site == (0, 0) else (0 if site == (1, 1) else 1)
            assert got[y, x, ch] == f[y, x]


# ---- parameter surface on RIP_DEVICE_NONE handles --------------------------------------------------------------------------
def test_default_set_get_and_reject(host_pipe):
    assert host_pipe.get_debayer_method() == "bilinear"
    host_pipe.set_debayer_method("mht")
    assert host_pipe.get_debayer_method() == "mht"
    with pytest.raises(ValueError) as e:
        host_pipe.set_debayer_method("vng")
    assert "'bilinear'" in str(e.value) and "'mht'" in str(e.value)
    assert host_pipe.get_debayer_method() == "mht"
    host_pipe.set_debayer_method("bilinear")
    assert host_pipe.get_debayer_method() == "bilinear"


def test_capacity_of_the_getter(rip_lib, host_pipe):
    import ctypes as C
    buf = C.create_string_buffer(4)
    assert rip_lib.rip_get_debayer_method(host_pipe._h, buf, C.c_size_t(4)) != 0  # "bilinear" needs 9 bytes


def write_params(tmp_path, text):
    path = tmp_path / "params.yaml"
    path.write_text(text)
    return str(path)


def test_yaml_key(tmp_path, host_pipe):
    host_pipe.load_params(write_params(tmp_path, "debayer:\n  enabled: true\n  method: mht\nflip:\n  enabled: true\n  angle: 90\n"))
    assert host_pipe.get_debayer_method() == "mht"
    # a file without the key re-creates the module with the default, as loadParams does for every key
    host_pipe.load_params(write_params(tmp_path, "debayer:\n  enabled: true\nflip:\n  enabled: true\n  angle: 90\n"))
    assert host_pipe.get_debayer_method() == "bilinear"


def test_yaml_unknown_method_fails_and_changes_nothing(tmp_path, host_pipe):
    host_pipe.set_debayer_method("mht")
    host_pipe.set_flip(True)
    host_pipe.set_flip_angle(180)
    before = host_pipe.query_output(20, 30, 1, "bayer_rggb8")
    with pytest.raises(ValueError) as e:
        host_pipe.load_params(write_params(tmp_path, "debayer:\n  method: vng\nflip:\n  enabled: false\n  angle: 90\n"))
    assert "'bilinear'" in str(e.value) and "'mht'" in str(e.value)
    assert host_pipe.get_debayer_method() == "mht"
    assert host_pipe.is_flip_enabled()
    assert host_pipe.query_output(20, 30, 1, "bayer_rggb8") == before


@pytest.mark.parametrize("encoding,channels", [("bayer_rggb8", 1), ("bayer_gbrg8", 1), ("bgr8", 3), ("mono8", 1), ("rgb8", 3)])
@pytest.mark.parametrize("angle", [0, 90, 180, 270])
def test_geometry_does_not_depend_on_the_method(host_pipe, encoding, channels, angle):
    host_pipe.set_flip(True)
    host_pipe.set_flip_angle(angle)
    got = {}
    for method in ("bilinear", "mht"):
        host_pipe.set_debayer_method(method)
        got[method] = (host_pipe.query_output(37, 52, channels, encoding), host_pipe.query_taps(37, 52, channels, encoding))
    assert got["bilinear"] == got["mht"]


def test_query_16bit_geometry(host_pipe):
    host_pipe.set_debayer_16bit(True)
    host_pipe.set_flip(True)
    host_pipe.set_flip_angle(90)
    host_pipe.set_white_balance(False)
    host_pipe.set_undistortion(False)
    a = host_pipe.query_output(20, 30, 1, "bayer_bggr16")
    host_pipe.set_debayer_method("mht")
    assert host_pipe.query_output(20, 30, 1, "bayer_bggr16") == a


def test_frontend_parameter_maps_to_the_handle(rip_lib):
    from raw_image_pipeline_amd import RawImagePipeline
    from raw_image_pipeline_amd.frontend import NODE_DEFAULTS, CameraStream
    assert NODE_DEFAULTS["debayer/method"] == "bilinear"
    cam = CameraStream({}, pipeline=RawImagePipeline(False, device=-1))
    assert cam.pipe.get_debayer_method() == "bilinear"
    cam = CameraStream({"debayer/method": "mht"}, pipeline=RawImagePipeline(False, device=-1))
    assert cam.pipe.get_debayer_method() == "mht"
    with pytest.raises(ValueError):
        CameraStream({"debayer/method": "edge_aware"}, pipeline=RawImagePipeline(False, device=-1))


def test_cpp_facade_calls_both_methods(tmp_path, rip_lib):
    src = os.path.join(ROOT, "tests", "cpp", "debayer_method_test.cpp")
    exe = str(tmp_path / "debayer_method_test")
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-DRIP_NO_OPENCV", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
           "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ)
    env["RIP_DEVICE"] = "-1"
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "debayer method OK" in r.stdout


def test_demosaic_source_has_no_scratch_or_spills():
    """hipcc -Rpass-analysis=kernel-resource-usage on rip_demosaic.hip: no private segment, no spilled registers."""
    from raw_image_pipeline_amd import build as B
    src = os.path.join(ROOT, "raw_image_pipeline_amd", "csrc", "rip_demosaic.hip")
    cmd = [B.hipcc()] + B.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-x", "hip", "-c", src, "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    kernels = r.stderr.count("Function Name:")
    assert kernels >= 17, r.stderr  # 16 tiled variants (4 patterns x 4 flips) + the 16-bit per-pixel kernel
    scratch = [l for l in r.stderr.splitlines() if "ScratchSize" in l]
    spills = [l for l in r.stderr.splitlines() if "Spill:" in l]
    assert len(scratch) == kernels and all(l.rstrip().endswith(" 0 [-Rpass-analysis=kernel-resource-usage]") for l in scratch), scratch
    assert spills and all(l.rstrip().endswith(" 0 [-Rpass-analysis=kernel-resource-usage]") for l in spills), spills
