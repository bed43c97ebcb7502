"""CLAHE on the delivered one-channel picture (include/rip.h rip_set_output_clahe; PARITY.md "Local contrast: CLAHE") without a GPU:
the definition's known answers and properties on tests/clahe_reference.py, the setter / getter / YAML keys per head, the queries,
refusals and masks on RIP_DEVICE_NONE handles, the C++ facade, and both kernels of csrc/rip_clahe.hip executed on the host phase by
phase against the reference -- plainly, and under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program.
Tolerance 0 wherever the library is compared."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import clahe_cases as CC
import clahe_reference as CL
from helpers import build_host_program
from raw_image_pipeline_amd import RawImagePipeline
from raw_image_pipeline_amd import pipeline as P
from test_cpp_facade import BRANCHES, run_env
from test_resize import write_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAYER = "bayer_rggb8"


# ---- the definition: known answers ------------------------------------------------------------------------------------------------
def ramp(h, w, step):
    return (step * np.arange(h * w)).astype(np.uint8).reshape(h, w)


def test_ka1_tiles_divide():
    pic = ramp(4, 8, 8)
    assert CL.geometry(4, 8, 2, 2, 2.0)[:5] == (4, 8, 4, 2, 1)
    want = [[32, 64, 96, 96, 80, 80, 96, 128], [159, 191, 223, 223, 207, 207, 223, 255], [144, 160, 176, 176, 168, 168, 176, 192],
            [159, 191, 223, 223, 207, 207, 223, 255]]
    assert CL.clahe(pic, 2.0, 2, 2).tolist() == want
    assert CL.clahe(pic, 0.0, 2, 2).tolist() == want


def test_ka2_neither_axis_divides():
    assert CL.geometry(5, 7, 2, 2, 4.0)[:5] == (6, 8, 4, 3, 1)
    assert CL.clahe(ramp(5, 7, 7), 4.0, 2, 2).tolist() == [
        [21, 42, 64, 69, 64, 69, 85], [106, 128, 149, 149, 138, 138, 170], [166, 184, 202, 203, 196, 199, 209], [170, 180, 192, 194, 197, 202, 212],
        [202, 219, 238, 242, 237, 242, 255]]


def test_ka3_a_dividing_axis_is_extended_too():
    assert CL.geometry(5, 8, 2, 2, 4.0)[:5] == (6, 10, 5, 3, 1)
    assert CL.clahe(ramp(5, 8, 6), 4.0, 2, 2).tolist() == [
        [17, 34, 51, 63, 65, 60, 61, 85], [102, 119, 136, 146, 144, 136, 146, 155], [162, 178, 193, 200, 197, 195, 195, 201],
        [162, 170, 187, 192, 196, 196, 198, 204], [184, 198, 227, 237, 238, 234, 245, 255]]


def test_ka4_flat_picture_and_the_residual():
    pic = np.full((16, 16), 100, np.uint8)
    assert CL.geometry(16, 16, 4, 4, 3.0)[2:5] == (4, 4, 1)
    assert (CL.clahe(pic, 3.0, 4, 4) == 112).all()
    lut = CL.luts(pic, 3.0, 4, 4)
    assert lut[0, 0, 99] == 96 and lut[0, 0, 100] == 112


def test_ka5_random_picture():
    pic = np.random.default_rng(1).integers(0, 256, (37, 53), dtype=np.uint8)
    assert CL.geometry(37, 53, 8, 8, 3.0)[:5] == (40, 56, 7, 5, 1)
    out = CL.clahe(pic, 3.0, 8, 8)
    assert int(out.astype(np.int64).sum()) == 258868
    assert out[0, :6].tolist() == [255, 233, 44, 124, 248, 172] and out[-1, -6:].tolist() == [15, 212, 64, 186, 79, 143]


# ---- the definition: properties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CC.SHAPES[:8], ids=lambda s: "%dx%d_%dx%d" % (s[0] + s[1]))
@pytest.mark.parametrize("clip", CC.CLIPS)
def test_every_lut_is_non_decreasing_and_ends_at_the_scaled_sum(shape, clip):
    (w, h), (tx, ty) = shape
    pic = CC.picture("random", h, w, seed=3)
    eh, ew, tw, th, cl, scale = CL.geometry(h, w, tx, ty, clip)
    lut = CL.luts(pic, clip, tx, ty).astype(np.int64)
    assert (np.diff(lut, axis=2) >= 0).all()
    # the closed form drops what of the residual does not fit below bin 256: the sum is the area, or less by that rest
    e = CL.extend(pic, eh, ew)
    for j in range(ty):
        for i in range(tx):
            hist = np.bincount(e[j * th:(j + 1) * th, i * tw:(i + 1) * tw].ravel(), minlength=256)
            total = tw * th
            if cl > 0:
                residual = int(np.maximum(hist - cl, 0).sum()) % 256
                if residual:
                    step = max(256 // residual, 1)
                    total -= residual - min(residual, (255 // step) + 1)
            assert lut[j, i, 255] == min(255, int(np.rint(np.float32(total) * scale)))
            if total == tw * th:
                assert lut[j, i, 255] == 255


@pytest.mark.parametrize("content", CC.CONTENTS)
def test_a_clip_limit_of_256_and_more_is_no_clipping(content):
    pic = CC.picture(content, 45, 67, seed=5)
    plain = CL.clahe(pic, 0.0, 4, 3)
    for clip in (256.0, 300.5, 1e9):
        assert np.array_equal(CL.clahe(pic, clip, 4, 3), plain)


@pytest.mark.parametrize("content", CC.CONTENTS)
def test_one_tile_without_a_clip_is_histogram_equalisation(content):
    pic = CC.picture(content, 48, 64, seed=7)
    out = CL.clahe(pic, 0.0, 1, 1).astype(np.float64)
    cdf = np.cumsum(np.bincount(pic.ravel(), minlength=256)).astype(np.float64) / pic.size
    assert np.abs(out - 255.0 * cdf[pic]).max() <= 1.0


def test_bands_do_not_take_part():
    img = CC.picture("random", 40, 60, seed=9)
    out = CL.apply_to_delivered(img, (6, 4, 48, 30), 3.0, 4, 4)
    inside = np.zeros(img.shape, bool)
    inside[4:34, 6:54] = True
    assert np.array_equal(out[~inside], img[~inside])
    assert np.array_equal(out[4:34, 6:54], CL.clahe(img[4:34, 6:54], 3.0, 4, 4))


# ---- setter, getter, YAML -----------------------------------------------------------------------------------------------------------
def test_setter_getter_per_head(host_pipe):
    p = host_pipe
    assert p.get_output_clahe() == (0.0, 0, 0)
    p.set_output_heads(3)
    values = ((3.0, 8, 8), (0.0, 16, 1), (1e9, 1, 16))
    for k, v in enumerate(values):
        p.select_output_head(k)
        p.set_output_clahe(*v)
    for k, v in enumerate(values):
        p.select_output_head(k)
        assert p.get_output_clahe() == v
    for bad in ((-0.5, 8, 8), (math.inf, 8, 8), (math.nan, 8, 8), (2.0, 0, 8), (2.0, 8, 0), (2.0, 17, 8), (2.0, 8, 17), (2.0, -1, -1), (-1.0, 0, 0)):
        with pytest.raises(ValueError, match="output clahe"):
            p.set_output_clahe(*bad)
        assert p.get_output_clahe() == (1e9, 1, 16)
    assert p._lib.rip_set_output_clahe(None, P.C.c_double(2.0), 8, 8) == P.RIP_ERR_INVALID_ARGUMENT
    assert p._lib.rip_get_output_clahe(p._h, None, None, None) == P.RIP_OK
    p.set_output_clahe(5.0, 0, 0)          # off keeps the clip limit it was given
    assert p.get_output_clahe() == (5.0, 0, 0)
    p.set_output_heads(1)                  # rip_set_output_heads resets it for the heads it resets
    p.set_output_heads(3)
    assert [p.select_output_head(k) or p.get_output_clahe() for k in range(3)] == [(3.0, 8, 8), (0.0, 0, 0), (0.0, 0, 0)]


def test_yaml_keys(tmp_path, host_pipe):
    p = host_pipe
    p.load_params(write_params(tmp_path, "output:\n  format: mono8\n  clahe_clip_limit: 3.0\n  clahe_tiles: [8, 8]\noutput_1:\n  format: rgb8\noutput_2:\n  clahe_tiles: [4, 2]\n"))
    assert p.get_output_heads() == 3
    for k, v in enumerate(((3.0, 8, 8), (0.0, 0, 0), (0.0, 4, 2))):
        p.select_output_head(k)
        assert p.get_output_clahe() == v
    p.load_params(write_params(tmp_path, "output:\n  format: mono8\n"))          # absent: off
    assert p.get_output_clahe() == (0.0, 0, 0) and p.get_output_format() == "mono8"


@pytest.mark.parametrize("text", ["output:\n  clahe_tiles: [8]\n", "output:\n  clahe_tiles: [0, 8]\n", "output:\n  clahe_tiles: [17, 17]\n", "output:\n  clahe_tiles: [2.5, 2]\n",
                                  "output:\n  clahe_clip_limit: -1\n  clahe_tiles: [8, 8]\n", "output:\n  format: mono8\noutput_1:\n  clahe_tiles: [8, 0]\n"])
def test_yaml_invalid_value_fails_and_changes_nothing(tmp_path, host_pipe, text):
    p = host_pipe
    p.set_output_clahe(2.0, 4, 4)
    p.set_flip(True)
    with pytest.raises(ValueError):
        p.load_params(write_params(tmp_path, "flip:\n  enabled: false\n" + text))
    assert p.get_output_clahe() == (2.0, 4, 4) and p.is_flip_enabled() and p.get_output_format() == "native"


@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade(tmp_path, rip_lib, branch):
    exe = str(tmp_path / ("clahe_test_" + branch.replace("-", "_")))
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror"] + BRANCHES[branch] + ["-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "clahe_test.cpp"), "-o", exe, "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir,
           "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "host"], capture_output=True, text=True, env=run_env(-1))
    assert r.returncode == 0 and "clahe host OK" in r.stdout, r.stdout + r.stderr


# ---- the queries on a handle without a device ---------------------------------------------------------------------------------------
GEOMETRIES = [dict(), dict(size=(64, 48)), dict(size=(64, 48), fit="letterbox"), dict(size=(64, 48), fit="crop"), dict(roi=(8, 4, 64, 32))]


def configure_geometry(p, g):
    p.set_output_size(*g.get("size", (0, 0)))
    p.set_output_fit(g.get("fit", "stretch"))
    p.set_output_roi(*g.get("roi", (0, 0, 0, 0)))


def new_host_pipe():
    p = RawImagePipeline(False, "", "", "", device=-1)
    for off in (p.set_undistortion, p.set_white_balance, p.set_vignetting_correction, p.set_color_calibration, p.set_gamma_correction,
                p.set_color_enhancer, p.set_flip):
        off(False)
    return p


def all_queries(p, rows, cols, channels, enc):
    return [lambda: p.query_output(rows, cols, channels, enc), lambda: p.query_output_bytes(rows, cols, channels, enc),
            lambda: p.get_output_camera_info(rows, cols, channels, enc), lambda: p.get_output_window(rows, cols, channels, enc)]


@pytest.mark.parametrize("frame", [(1, BAYER, "mono8"), (1, "mono8", "native"), (1, "mono8", "mono8")], ids=["bayer-mono8", "mono-native", "mono-mono8"])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=["plain", "target", "letterbox", "crop", "window"])
def test_what_describes_the_delivered_image_does_not_change(rip_lib, frame, geometry):
    channels, enc, fmt = frame
    p, twin = new_host_pipe(), new_host_pipe()
    for q in (p, twin):
        configure_geometry(q, geometry)
        q.set_output_format(fmt)
        q.set_rect_mask("coverage")
    p.set_output_clahe(3.0, 8, 8)
    for a, b in zip(all_queries(p, 72, 136, channels, enc), all_queries(twin, 72, 136, channels, enc)):
        got, want = a(), b()
        assert all(np.array_equal(x, y) for x, y in zip(got, want)), (got, want)
    sizes = []
    for q in (p, twin):
        h, w = P.C.c_int(), P.C.c_int()
        assert q._lib.rip_get_output_mask(q._h, 72, 136, channels, enc.encode(), None, P.C.c_size_t(0), P.C.byref(h), P.C.byref(w)) == P.RIP_OK
        sizes.append((h.value, w.value))
    assert sizes[0] == sizes[1] == p.query_output(72, 136, channels, enc)[:2]
    assert p.get_processed_image().size == 0


def test_refusals_and_their_order(rip_lib):
    p = new_host_pipe()
    p.set_output_clahe(3.0, 8, 8)
    # (a) more than one channel: a colour result under native, rgb8, a planar and a YUV format; the message names mono8
    for fmt in ("native", "rgb8", "rgb_chw_f32", "bgr_chw_f16", "nv12", "i420"):
        p.set_output_format(fmt)
        for q in all_queries(p, 72, 136, 1, BAYER):
            with pytest.raises(ValueError, match="output clahe needs a delivered one-channel.*'mono8'"):
                q()
    for q in all_queries(p, 72, 136, 3, "bgr8"):
        with pytest.raises(ValueError, match="output clahe needs a delivered one-channel"):
            q()
    # ... behind every existing refusal of that head: the format's own rules, the YUV format's odd size, the resize's
    p.set_output_format("rgb8")
    for q in all_queries(p, 33, 65, 1, "mono8"):
        with pytest.raises(ValueError, match="needs a three-channel pipeline result"):
            q()
    p.set_output_format("nv12")
    for q in all_queries(p, 71, 135, 1, BAYER):
        with pytest.raises(ValueError, match="even width and height"):
            q()
    p.set_output_format("mono8")
    p.set_output_roi(100, 0, 64, 32)
    for q in all_queries(p, 72, 136, 1, BAYER):
        with pytest.raises(ValueError) as e:
            q()
        assert "clahe" not in str(e.value)
    p.set_output_roi(0, 0, 0, 0)
    # a bgr16 result: the format's refusal first, (a) under native
    p.set_debayer_16bit(True)
    for q in all_queries(p, 72, 136, 1, "bayer_rggb16"):
        with pytest.raises(ValueError, match="needs an 8-bit pipeline result"):
            q()
    p.set_output_format("native")
    for q in all_queries(p, 72, 136, 1, "bayer_rggb16"):
        with pytest.raises(ValueError, match="output clahe needs a delivered one-channel"):
            q()
    # (b) a tile must hold two pixels per side: the picture, not the delivered image
    p.set_output_format("mono8")
    assert p.query_output(16, 16, 1, "mono8") == (16, 16, 1, "mono8")
    for rows, cols in ((15, 16), (16, 15), (15, 15)):
        for q in all_queries(p, rows, cols, 1, "mono8"):
            with pytest.raises(ValueError, match="output clahe: the delivered picture of %d x %d is smaller than two pixels per tile" % (cols, rows)):
                q()
    p.set_output_size(64, 64)
    p.set_output_fit("letterbox")          # 136 x 72 into 64 x 64: a picture of 64 x 34, bands above and below
    assert p.get_output_window(72, 136, 1, BAYER)[1] == (0, 15, 64, 34)
    p.set_output_clahe(3.0, 8, 16)
    assert p.query_output(72, 136, 1, BAYER) == (64, 64, 1, "mono8")
    p.set_output_size(56, 64)              # a picture of 56 x 30: lower than 2 x 16 rows, while the delivered image is not
    p.set_output_clahe(3.0, 0, 0)
    w, h = p.get_output_window(72, 136, 1, BAYER)[1][2:]
    p.set_output_clahe(3.0, 8, 16)
    assert (w, h) == (56, 30)
    for q in all_queries(p, 72, 136, 1, BAYER):
        with pytest.raises(ValueError, match="the delivered picture of %d x %d" % (w, h)):
            q()
    # (a) before (b)
    p.set_output_format("rgb8")
    with pytest.raises(ValueError, match="one-channel"):
        p.query_output(72, 136, 1, BAYER)
    # the heads calls name the head
    p.set_output_size(0, 0)
    p.set_output_fit("stretch")
    p.set_output_format("mono8")
    p.set_output_heads(2)
    p.select_output_head(1)
    p.set_output_clahe(2.0, 4, 4)
    with pytest.raises(ValueError, match="output head 1: output clahe needs"):
        p._head_queries([0, 1], 72, 136, 1, BAYER)
    # off: no refusal, whatever the clip limit
    p.set_output_clahe(2.0, 0, 0)
    assert p._head_queries([1], 72, 136, 1, BAYER)[1][:4] == (72, 136, 3, "bgr8")


def test_the_masks_do_not_see_it(rip_lib):
    """The mask queries of a handle without a device refuse what they refused and report the size they reported."""
    p, twin = new_host_pipe(), new_host_pipe()
    for q in (p, twin):
        q.set_output_format("mono8")
        q.set_output_size(64, 48)
        q.set_output_fit("letterbox")
    p.set_output_clahe(3.0, 4, 4)
    for mode in ("off", "coverage", "valid"):
        results = []
        for q in (p, twin):
            q.set_rect_mask(mode)
            h, w = P.C.c_int(), P.C.c_int()
            st = q._lib.rip_get_output_mask(q._h, 72, 136, 1, BAYER.encode(), None, P.C.c_size_t(0), P.C.byref(h), P.C.byref(w))
            results.append((st, h.value, w.value))
        assert results[0] == results[1], mode


# ---- the kernels on the host ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_kernels_run_on_the_host_equal_the_reference_byte_for_byte(tmp_path, sanitize):
    """tests/cpp/clahe_kernel_host.cpp: csrc/rip_clahe.hip compiled as host code with the toolchain's clang++; per workgroup of a
    launcher's grid a heap block of exactly the launch's LDS size and the kernel's phases one after another, each for all 256 threads;
    frames, tables and destinations in exactly sized heap blocks, destinations with sentinels.  The second build adds
    -fsanitize=address,undefined to this stand-alone program (no access outside a frame, a table block or the LDS block, no misaligned
    wide access, no signed overflow)."""
    exe = build_host_program(tmp_path, "clahe_kernel_host", ["clahe_kernel_host.cpp"], stub="hip_host_stub_lds", sanitize=sanitize,
                             extra=["-ffp-contract=off", "-Wno-unused-function", "-lm"])
    cases = CC.host_cases()
    assert len(cases) >= 50 and {c.in_place for c in cases} == {0, 1} and {c.offset for c in cases} >= {0, 1, 2, 3}
    assert {(c.width, c.height) for c in cases} >= {s for s, _ in CC.SHAPES} | {CC.LARGE_SHAPE[0]} and {c.clip for c in cases} == set(CC.CLIPS)
    cases_path, out_path = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    wants = []
    with open(cases_path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for i, c in enumerate(cases):
            f.write(struct.pack("<9id", c.height, c.width, c.tiles_x, c.tiles_y, c.frames, c.in_place, c.pad, c.offset, c.gap, c.clip))
            step = c.width + c.pad
            frame = step * c.height + c.gap
            want = np.full(c.offset + frame * (c.frames - 1) + step * (c.height - 1) + c.width, 0xA5, np.uint8)
            tables = []
            for k in range(c.frames):
                pic = CC.picture(c.content, c.height, c.width, seed=10 * i + k)
                f.write(pic.tobytes())
                rows = want[c.offset + k * frame:][:step * (c.height - 1) + c.width]
                rows = np.lib.stride_tricks.as_strided(rows, (c.height, c.width), (step, 1))
                rows[...] = CL.clahe(pic, c.clip, c.tiles_x, c.tiles_y)
                tables.append(CL.luts(pic, c.clip, c.tiles_x, c.tiles_y).ravel())
            wants.append(np.concatenate([want] + tables))
    r = subprocess.run([exe, cases_path, out_path], capture_output=True, text=True)
    assert r.returncode == 0 and "%d cases, 0 bad" % len(cases) in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.fromfile(out_path, np.uint8)
    at = 0
    for c, want in zip(cases, wants):
        assert np.array_equal(got[at:at + want.size], want), "%r: %d bytes differ" % (c, int((got[at:at + want.size] != want).sum()))
        at += want.size
    assert at == got.size
