"""Valid-pixel masks (include/rip.h rip_set_rect_mask, rip_get_output_mask; PARITY.md "Rect mask") without a GPU: defaults, the setter
and getter, the YAML key, the C++ facade, the geometry and the refusals of rip_get_output_mask against rip_query_output for every head
set of tests/heads_cases.py, and the kernels of csrc/rip_mask.hip executed on the host thread by thread against the oracle's remap of
a white image -- plainly, and under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program.  Everything at tolerance 0."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import heads_cases as HC
import mask_cases as MC
from helpers import build_host_program
from raw_image_pipeline_amd import RawImagePipeline
from raw_image_pipeline_amd import pipeline as P
from test_cpp_facade import BRANCHES, run_env
from test_resize import write_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("off", "coverage", "valid")


def output_mask_status(p, rows, cols, channels, encoding, out=None, capacity=0):
    """(status, message, height, width) of a raw rip_get_output_mask call."""
    h, w = C.c_int(-1), C.c_int(-1)
    st = p._lib.rip_get_output_mask(p._h, rows, cols, channels, encoding, out, C.c_size_t(capacity), C.byref(h), C.byref(w))
    return st, p._lib.rip_last_error(p._h).decode(), h.value, w.value


def query_status(p, rows, cols, channels, encoding):
    r, c, k = C.c_int(), C.c_int(), C.c_int()
    enc = C.create_string_buffer(32)
    st = p._lib.rip_query_output(p._h, rows, cols, channels, encoding, C.byref(r), C.byref(c), C.byref(k), enc)
    return st, p._lib.rip_last_error(p._h).decode(), r.value, c.value


# ---- defaults, setter, getter -----------------------------------------------------------------------------------------------
def test_defaults(host_pipe):
    p = host_pipe
    assert p.get_rect_mask_mode() == "off"
    assert p.get_rect_mask().shape == (0, 0)
    st, msg, _, _ = output_mask_status(p, 72, 136, 1, b"bayer_rggb8")
    assert st == P.RIP_ERR_INVALID_ARGUMENT and "'off'" in msg
    with pytest.raises(ValueError, match="'off'"):
        p.get_output_mask(72, 136, 1, "bayer_rggb8")
    with pytest.raises(ValueError, match="'off'"):
        p.get_output_mask_device(72, 136, 1, "bayer_rggb8")
    assert p.debug_rect_mask_info(0) == (0, 0)
    with pytest.raises(ValueError):
        p.debug_rect_mask_info(1)
    # the view of the empty image: geometry 0 and a null pointer
    view, r, c, k = C.c_void_p(1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert p._lib.rip_get_image_view(p._h, P.IMAGE_RECT_MASK, C.byref(view), C.byref(r), C.byref(c), C.byref(k)) == P.RIP_OK
    assert (view.value, r.value, c.value, k.value) == (None, 0, 0, 0)


def test_setter_and_getter(host_pipe):
    p = host_pipe
    for mode in ("coverage", "valid", "off", "valid", "coverage"):
        p.set_rect_mask(mode)
        assert p.get_rect_mask_mode() == mode
    for bad in ("on", "Coverage", "", "valid ", "binary"):
        with pytest.raises(ValueError, match="'off', 'coverage', 'valid'"):
            p.set_rect_mask(bad)
        assert p.get_rect_mask_mode() == "coverage"
    lib = p._lib
    assert lib.rip_set_rect_mask(p._h, None) == P.RIP_ERR_INVALID_ARGUMENT and p.get_rect_mask_mode() == "coverage"
    assert lib.rip_set_rect_mask(None, b"valid") == P.RIP_ERR_INVALID_ARGUMENT
    # no frame yet: the rect mask stays empty under every mode
    for mode in MODES:
        p.set_rect_mask(mode)
        assert p.get_rect_mask().shape == (0, 0)


def test_yaml_key(tmp_path, host_pipe):
    p = host_pipe
    p.set_rect_mask("valid")
    p.load_params(write_params(tmp_path, "undistortion:\n  enabled: true\n"))          # absent: off -- loadParams re-creates the module
    assert p.get_rect_mask_mode() == "off"
    for mode in MODES:
        p.load_params(write_params(tmp_path, "undistortion:\n  enabled: true\n  mask: %s\n" % mode))
        assert p.get_rect_mask_mode() == mode
    p.load_params(write_params(tmp_path, "flip:\n  enabled: false\n"))
    assert p.get_rect_mask_mode() == "off"


@pytest.mark.parametrize("bad", ["masked", "on", "[1, 2]", "255"])
def test_yaml_invalid_value_fails_and_changes_nothing(tmp_path, host_pipe, bad):
    p = host_pipe
    p.set_rect_mask("coverage")
    p.set_flip(True)
    with pytest.raises(ValueError):
        p.load_params(write_params(tmp_path, "flip:\n  enabled: false\nundistortion:\n  mask: %s\n" % bad))
    assert p.get_rect_mask_mode() == "coverage" and p.is_flip_enabled()


@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade(tmp_path, rip_lib, branch):
    exe = build_facade_program(tmp_path, branch)
    r = subprocess.run([exe, "host"], capture_output=True, text=True, env=run_env(-1))
    assert r.returncode == 0 and "mask host OK" in r.stdout, r.stdout + r.stderr


def build_facade_program(tmp_path, branch):
    exe = str(tmp_path / ("mask_test_" + branch.replace("-", "_")))
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror"] + BRANCHES[branch] + ["-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "mask_test.cpp"), "-o", exe, "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir,
           "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_front_end_lists_the_mask_topic_only_when_it_publishes_it():
    from raw_image_pipeline_amd.frontend import NODE_DEFAULTS, CameraStream
    assert NODE_DEFAULTS["rect_mask"] == "off"
    host = lambda: RawImagePipeline(False, device=-1)
    cam = CameraStream({"undistortion/enabled": True}, pipeline=host())
    assert cam.pipe.get_rect_mask_mode() == "off" and "/camera/image_mask" not in cam.topics()
    cam = CameraStream({"undistortion/enabled": True, "rect_mask": "valid", "output_prefix": "/alphasense/cam3"}, pipeline=host())
    assert cam.pipe.get_rect_mask_mode() == "valid"
    assert cam.topics()[:3] == ["/alphasense/cam3/color_rect/image", "/alphasense/cam3/color_rect/image/slow", "/alphasense/cam3/image_mask"]
    cam = CameraStream({"undistortion/enabled": False, "rect_mask": "coverage"}, pipeline=host())      # no rect image, no mask of it
    assert not [t for t in cam.topics() if "image_mask" in t]
    with pytest.raises(ValueError):
        CameraStream({"rect_mask": "both"}, pipeline=host())


# ---- geometry and refusals of rip_get_output_mask ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["coverage", "valid"])
@pytest.mark.parametrize("head_set", HC.SETS, ids=HC.set_id)
def test_geometry_equals_query_output_under_each_selection(host_pipe, head_set, mode):
    p = host_pipe
    f = HC.FRAMES[head_set.frame]
    HC.configure_pipeline(p, head_set.frame)
    HC.configure_heads(p, head_set.heads)
    p.set_rect_mask(mode)
    for k in reversed(range(len(head_set.heads))):
        p.select_output_head(k)
        rows, cols = p.query_output(f.size[1], f.size[0], f.channels, f.encoding)[:2]
        st, msg, h, w = output_mask_status(p, f.size[1], f.size[0], f.channels, f.encoding.encode())
        assert st == P.RIP_OK and (h, w) == (rows, cols), (k, msg)
        # null geometry pointers are fine too
        assert p._lib.rip_get_output_mask(p._h, f.size[1], f.size[0], f.channels, f.encoding.encode(), None, C.c_size_t(0), None, None) == P.RIP_OK
        # bytes need a device -- after the capacity, which is checked without one
        buf = (C.c_uint8 * (rows * cols))()
        st, msg, _, _ = output_mask_status(p, f.size[1], f.size[0], f.channels, f.encoding.encode(), buf, rows * cols - 1)
        assert st == P.RIP_ERR_CAPACITY and str(rows * cols) in msg, (k, msg)
        st, msg, _, _ = output_mask_status(p, f.size[1], f.size[0], f.channels, f.encoding.encode(), buf, rows * cols)
        assert st == P.RIP_ERR_DEVICE, (k, msg)
    assert p.debug_rect_mask_info(0) == (0, 0)          # nothing was built


def test_refusals_and_their_order(host_pipe):
    """First the mode off, then exactly the refusals of rip_query_output -- same status, same message --, then the capacity."""
    p = host_pipe
    HC.configure_pipeline(p, "bayer136")
    HC.configure_heads(p, (HC.IDENTITY, HC.Head(size=(300, 100), interp="area"), HC.Head(roi=(100, 0, 64, 32)), HC.Head(format="rgb8")))
    frames = [(72, 136, 1, b"bayer_rggb8"), (72, 136, 1, b"bayer_xxxx8"), (72, 136, 1, b"mono8"), (72, 136, 2, b"bgr8"), (0, 136, 1, b"bayer_rggb8"),
              (2, 2, 1, b"bayer_rggb8"), (72, 136, 1, b"bayer_rggb16")]
    tiny = (C.c_uint8 * 1)()
    for k in range(4):
        p.select_output_head(k)
        for frame in frames:
            p.set_rect_mask("off")
            st, msg, _, _ = output_mask_status(p, *frame, tiny, 1)
            assert st == P.RIP_ERR_INVALID_ARGUMENT and "'off'" in msg, (k, frame)          # the mode comes first, whatever else is wrong
            p.set_rect_mask("coverage")
            want = query_status(p, *frame)
            got = output_mask_status(p, *frame, tiny, 1)
            if want[0] != P.RIP_OK:
                assert got[:2] == want[:2], (k, frame, got, want)                            # the query's refusal, before the capacity
            else:
                assert got[0] == P.RIP_ERR_CAPACITY, (k, frame, got)
                assert output_mask_status(p, *frame)[2:] == want[2:]
    refused = []
    for k in range(4):
        p.select_output_head(k)
        refused.append(query_status(p, 72, 136, 1, b"bayer_rggb8")[0] != P.RIP_OK)
    assert refused == [False, True, True, False]       # the cases above did meet refusals of the heads' own settings
    st, msg, _, _ = output_mask_status(p, 72, 136, 1, None)
    assert st == P.RIP_ERR_INVALID_ARGUMENT and "encoding" in msg
    assert p._lib.rip_get_output_mask(None, 72, 136, 1, b"mono8", None, C.c_size_t(0), None, None) == P.RIP_ERR_INVALID_ARGUMENT
    d, pitch = C.c_void_p(), C.c_size_t()
    p.select_output_head(0)
    assert p._lib.rip_get_output_mask_device(p._h, 72, 136, 1, b"bayer_rggb8", C.byref(d), C.byref(pitch), None, None) == P.RIP_ERR_DEVICE
    assert p._lib.rip_get_output_mask_device(p._h, 72, 136, 1, b"bayer_rggb8", None, None, None, None) == P.RIP_ERR_INVALID_ARGUMENT


# ---- the kernels, executed on the host ---------------------------------------------------------------------------------------
def host_cases(O):
    """(drows, dcols, src_rows, src_cols, binary, pitch, dst offset, map phase, map_x, map_y, label, (balance, fov_scale) or None)"""
    out = []

    def add(mx, my, src, label, pair=None):
        drows, dcols = mx.shape
        odd = dcols + 1 if dcols % 2 == 0 else dcols + 2
        for binary in (0, 1):
            for i, (pitch, off) in enumerate(((dcols, 0), ((dcols + 15) // 16 * 16, 0), (odd, 1))):
                out.append((drows, dcols, src[1], src[0], binary, pitch, off, 8 * ((len(out) + i) % 2), mx, my, label, pair))
    for size in MC.SIZES:
        for pair in MC.PAIRS:
            mx, my = MC.fisheye_maps(O, size, pair)
            add(mx, my, size, "fisheye %s %s" % (size, pair), pair)
    for size, src in MC.OTHER_SOURCES:
        mx, my = MC.fisheye_maps(O, size, (1.0, 1.0))
        add(mx, my, src, "fisheye %s source %s" % (size, src))
    for src in MC.HAND_SOURCES:
        for phase, width in enumerate(MC.HAND_WIDTHS):
            mx, my = MC.hand_maps(width, src, phase)
            add(mx, my, src, "hand-made width %d source %s" % (width, src))
    return out


def test_the_expectations_hold_every_class(oracle):
    """What the cases promise of the oracle's masks, so that a constant mask cannot pass any of them."""
    for size in MC.SIZES:
        for pair in MC.PAIRS:
            MC.assert_classes(MC.expected(oracle, *MC.fisheye_maps(oracle, size, pair), size), pair, "%s %s" % (size, pair))
    assert MC.classes(MC.expected(oracle, *MC.fisheye_maps(oracle, (200, 136), (1.0, 1.0)), (200, 136))) == (4076, 461, 22663)
    for size, src in MC.OTHER_SOURCES:
        z, part, full = MC.classes(MC.expected(oracle, *MC.fisheye_maps(oracle, size, (1.0, 1.0)), src))
        assert z > 0 and part > 0 and full > 0, (size, src)
    for src in MC.HAND_SOURCES:
        seen = set()
        for phase, width in enumerate(MC.HAND_WIDTHS):
            seen |= set(np.unique(MC.expected(oracle, *MC.hand_maps(width, src, phase), src)).tolist())
        assert {0, 255} <= seen and seen - {0, 255}, (src, sorted(seen))          # outside, inside and partly covered entries


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_kernels_run_on_the_host_equal_the_oracles_remap_of_white(tmp_path, oracle, sanitize):
    """tests/cpp/mask_kernel_host.cpp: csrc/rip_mask.hip compiled as host code with the toolchain's clang++, every thread of the
    launcher's grid run in turn from exactly sized maps into exactly sized masks with sentinels behind every row, at tight, 16-byte and
    odd pitches, BINARY both ways.  The second build adds -fsanitize=address,undefined to this stand-alone program (no
    out-of-bounds access, no misaligned wide access)."""
    exe = build_host_program(tmp_path, "mask_kernel_host", ["mask_kernel_host.cpp"], sanitize=sanitize, extra=["-ffp-contract=off", "-Wall"])
    cases = host_cases(oracle)
    assert len(cases) == 6 * (16 + 3 + 2 * 13)
    cases_path, out_path = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(cases_path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            f.write(struct.pack("<8i", *c[:8]))
            f.write(np.ascontiguousarray(np.stack([c[8], c[9]], axis=-1), np.float32).tobytes())
    r = subprocess.run([exe, cases_path, out_path], capture_output=True, text=True)
    assert r.returncode == 0 and "%d cases, 0 bad" % len(cases) in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.fromfile(out_path, np.uint8)
    at = 0
    expectations = {}
    for (drows, dcols, srows, scols, binary, pitch, off, _, mx, my, label, pair) in cases:
        key = (label, srows, scols)
        if key not in expectations:          # one remap per map and source, shared by its six layouts
            expectations[key] = MC.expected(oracle, mx, my, (scols, srows))
            if pair is not None:
                MC.assert_classes(expectations[key], pair, label)
        m = expectations[key]
        total = off + pitch * (drows - 1) + dcols
        want = np.full(total, 0xA5, np.uint8)
        rows = MC.valid_of(m) if binary else m
        for y in range(drows):
            want[off + y * pitch:off + y * pitch + dcols] = rows[y]
        what = "%s, binary %d, pitch %d, offset %d" % (label, binary, pitch, off)
        assert np.array_equal(got[at:at + total], want), "%s: %d bytes differ" % (what, int((got[at:at + total] != want).sum()))
        at += total
    assert at == got.size
