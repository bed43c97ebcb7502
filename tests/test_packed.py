"""Packed 10- and 12-bit Bayer frames (include/rip.h "Packed Bayer frames") without a GPU: the layouts' known answers, the
numpy pack / unpack pair, the kernel's extract functions through rip_debug_unpack, geometry queries and error cases on
RIP_DEVICE_NONE handles, the width inference of the Python layer, the front end, the C++ facade, the fuzz generator of
tests/test_packed_gpu.py, and what the compiler made of rip_packed.hip."""
import os
import subprocess
import sys

import numpy as np
import pytest

import packed_cases as PC
import packed_reference as R
import raw16_cases as G
from helpers import LAYOUTS as BATCH_LAYOUTS
from raw_image_pipeline_amd import RipAssertError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_NAMES = [R.enc(name, layout) for name in R.NAMES for layout in R.LAYOUTS]

KNOWN = [("10p", [0x3FF, 0, 0x155, 0x2AA], "FF 03 50 95 AA"), ("10_csi2", [0x3FF, 0, 0x155, 0x2AA], "FF 00 55 AA 93"),
         ("12p", [0xABC, 0x123], "BC 3A 12"), ("12_csi2", [0xABC, 0x123], "AB 12 3C")]


# ---- the layouts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,samples,hexbytes", KNOWN)
def test_known_answers(rip_lib, layout, samples, hexbytes):
    want = np.array([samples], np.uint16)
    raw = np.frombuffer(bytes.fromhex(hexbytes), np.uint8).reshape(1, -1)
    assert np.array_equal(R.pack(want, layout), raw)
    assert np.array_equal(R.unpack(raw, len(samples), layout), want)
    st, got = R.lib_unpack(rip_lib, R.enc("rggb", layout), raw, len(samples))
    assert st == 0 and np.array_equal(got, want)


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_unpack_inverts_pack_at_every_width(layout):
    rng = np.random.default_rng(R.BITS[layout])
    widths = [w for w in range(3, 71) if w % R.WIDTH_MULTIPLE[layout] == 0]
    assert widths[0] <= 4 and widths[-1] >= 68
    for w in widths:
        x = rng.integers(0, 1 << R.BITS[layout], (5, w)).astype(np.uint16)
        for fill in (0, 1):
            p = R.pack(x, layout, fill_bits=fill)
            assert p.shape == (5, R.row_bytes(w, layout)) and p.dtype == np.uint8
            assert np.array_equal(R.unpack(p, w, layout), x), (layout, w)


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_the_kernels_extract_equals_unpack_for_every_value_at_every_position(rip_lib, layout):
    """rip_debug_unpack -- the extract functions of the kernel's byte path -- on rows that hold every sample value at every
    position of a group, with random neighbours, at a tight and two padded pitches, with garbage in the trailing bits of the
    last byte and in the padding."""
    bits, group = R.BITS[layout], R.GROUP[layout]
    n = 1 << bits
    rng = np.random.default_rng(bits * 7 + group)
    cols = 4 * group + (3 if R.WIDTH_MULTIPLE[layout] == 1 else 0)   # p layouts: a width whose last byte has spare bits
    seen = np.zeros((n, group), bool)
    frame = rng.integers(0, n, (n * group, cols)).astype(np.uint16)
    for pos in range(group):
        frame[pos * n:(pos + 1) * n, group + pos] = np.arange(n)       # every value at position x mod group == pos
    for fill in (0, 1):
        packed = R.pack(frame, layout, fill_bits=fill)
        for pad, junk in ((0, 0), (1, 0xFF), (7, 0x5A)):
            view, wide = R.pitched(packed, packed.shape[1] + pad, junk)
            st, got = R.lib_unpack(rip_lib, R.enc("grbg", layout), view, cols)
            assert st == 0
            bad = np.argwhere(got != frame)
            assert bad.size == 0, "%s fill %d pad %d: sample (%d, %d) = %d, expected %d" % (
                layout, fill, pad, bad[0][0], bad[0][1], got[tuple(bad[0])], frame[tuple(bad[0])])
            assert np.array_equal(got, R.unpack(wide, cols, layout))
    for pos in range(group):
        seen[frame[pos * n:(pos + 1) * n, group + pos], pos] = True
    assert seen.all()


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_debug_unpack_error_cases(rip_lib, layout):
    cols = 8
    raw = np.zeros((3, R.row_bytes(cols, layout)), np.uint8)
    assert R.lib_unpack(rip_lib, R.enc("rggb", layout), raw, cols)[0] == 0
    assert R.lib_unpack(rip_lib, R.enc("rggb", layout), raw, cols, step=raw.shape[1] - 1)[0] == 1   # step below a row
    assert R.lib_unpack(rip_lib, "bayer_rggb16", raw, cols)[0] == 1
    assert R.lib_unpack(rip_lib, "bayer_rgbg" + layout, raw, cols)[0] == 1
    if R.WIDTH_MULTIPLE[layout] > 1:
        assert R.lib_unpack(rip_lib, R.enc("rggb", layout), raw, cols - 1)[0] == 1


# ---- geometry queries and error cases on RIP_DEVICE_NONE handles ------------------------------------------------------------------
@pytest.mark.parametrize("encoding", ALL_NAMES)
def test_query_output_and_taps(host_pipe, encoding):
    """On the parent commit these names fell through to the mono path: one channel and the name echoed back."""
    p = host_pipe
    assert p.query_output(48, 64, 1, encoding) == (48, 64, 3, "bgr8")
    assert p.query_taps(48, 64, 1, encoding) == (48, 64, 3)
    p.set_flip(True)
    p.set_flip_angle(90)
    assert p.query_output(48, 64, 1, encoding) == (64, 48, 3, "bgr8")
    assert p.query_taps(48, 64, 1, encoding) == (64, 48, 3)
    # never bgr16, whatever the 16-bit switches say; every 8-bit stage is allowed
    for opt_in in (False, True):
        for rng in ((0, 0), (64, 1023)):
            p.set_debayer_16bit(opt_in)
            p.set_debayer_16bit_range(*rng)
            p.set_gamma_correction(True)
            p.set_debayer_method("mht" if opt_in else "bilinear")
            assert p.query_output(48, 64, 1, encoding) == (64, 48, 3, "bgr8")
            assert p.get_debayer_16bit_range() == rng


@pytest.mark.parametrize("encoding", ALL_NAMES)
def test_error_cases(host_pipe, encoding):
    p = host_pipe
    with pytest.raises(RipAssertError):
        p.query_output(48, 64, 3, encoding)
    with pytest.raises(RipAssertError):
        p.query_output(2, 2, 1, encoding)
    with pytest.raises(RipAssertError):
        p.query_output(2, 64, 1, encoding)
    layout = encoding[10:]
    m = R.WIDTH_MULTIPLE[layout]
    for cols in range(61, 69):
        if cols % m == 0:
            assert p.query_output(48, cols, 1, encoding) == (48, cols, 3, "bgr8")
        else:
            with pytest.raises(ValueError, match="multiple of %d" % m):
                p.query_output(48, cols, 1, encoding)


def test_no_other_name_changes_meaning(host_pipe):
    p = host_pipe
    assert p.query_output(48, 64, 1, "mono8") == (48, 64, 1, "mono8")
    assert p.query_output(48, 64, 1, "bayer_rggb14p") == (48, 64, 1, "bayer_rggb14p")   # still the mono path
    assert p.query_output(48, 64, 1, "bayer_rggb10") == (48, 64, 1, "bayer_rggb10")
    assert p.query_output(48, 64, 1, "bayer_rggb8") == (48, 64, 3, "bgr8")
    with pytest.raises(ValueError, match="valid pattern but is not supported"):
        p.query_output(48, 64, 1, "bayer_rggb16")


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_width_inference_is_exact_for_tight_rows(layout):
    from raw_image_pipeline_amd.pipeline import packed_bits, packed_width
    assert packed_bits(R.enc("gbrg", layout)) == R.BITS[layout]
    for w in range(1, 5000):
        assert packed_width(R.row_bytes(w, layout), R.BITS[layout]) == w
    assert packed_bits("bayer_rggb8") == 0 and packed_bits("bayer_rggb16") == 0 and packed_bits("mono8") == 0 and packed_bits("bayer_xxxx10p") == 0


def test_python_layer_checks_the_frame(host_pipe):
    p = host_pipe
    with pytest.raises(ValueError, match="2-D uint8"):
        p.process(np.zeros((8, 10), np.uint16), "bayer_rggb10p")
    with pytest.raises(ValueError, match="2-D uint8"):
        p.submit(np.zeros((8, 10, 1), np.uint8), "bayer_rggb10p")
    with pytest.raises(ValueError, match="do not hold"):
        p.process(np.zeros((8, 10), np.uint8), "bayer_rggb10p", width=9)     # 9 pixels need 12 bytes
    with pytest.raises(ValueError, match="packed Bayer encodings only"):
        p.process(np.zeros((8, 10), np.uint8), "bayer_rggb8", width=10)
    with pytest.raises(ValueError, match="multiple of 4"):
        p.process(np.zeros((8, 10), np.uint8), "bayer_rggb10_csi2", width=6)
    # accepted up to the device: a parameter-only handle refuses the frame call itself
    with pytest.raises(Exception, match="device"):
        p.process(np.zeros((8, 10), np.uint8), "bayer_rggb10p")


def test_frontend_forwards_the_width_and_the_levels(rip_lib):
    from raw_image_pipeline_amd import RawImagePipeline
    from raw_image_pipeline_amd.frontend import CameraStream
    cam = CameraStream({"debayer/black_level": 256, "debayer/white_level": 4095}, pipeline=RawImagePipeline(False, device=-1))
    assert cam.pipe.get_debayer_16bit_range() == (256, 4095)
    assert cam.pipe.query_output(20, 30, 1, "bayer_rggb12p") == (20, 30, 3, "bgr8")
    frame = np.zeros((20, 48), np.uint8)
    for call in (cam.on_image, cam.submit, cam.on_image_pipelined):
        with pytest.raises(ValueError, match="do not hold"):
            call(frame, "bayer_rggb12p", width=40)   # reached the pipeline's check: 40 pixels need 60 bytes


# ---- the fuzz generator of tests/test_packed_gpu.py ---------------------------------------------------------------------------------
def test_fuzz_generator_only_produces_valid_cases(host_pipe):
    from helpers import configure
    cases = [PC.fuzz_case(s) for s in range(PC.N_FUZZ)]
    assert len(cases) == PC.N_FUZZ >= 40
    for case in cases:
        layout = case["layout"]
        black, white = PC.effective_range(layout, case["range"])
        assert 0 <= black < white <= 65535
        assert case["w"] >= 3 and case["h"] >= 3 and case["w"] % R.WIDTH_MULTIPLE[layout] == 0 and case["n"] >= 1
        configure(host_pipe, dict(case["c"], cam=None))
        host_pipe.set_debayer_method(case["method"])
        if case["range"] is not None:
            host_pipe.set_debayer_16bit_range(*case["range"])
        ow, oh = (case["h"], case["w"]) if case["flip"] in (90, 270) else (case["w"], case["h"])
        assert host_pipe.query_taps(case["h"], case["w"], 1, R.enc(case["name"], layout)) == (oh, ow, 3)
        frame = PC.gen_samples(case["w"], case["h"], case["name"], case["seed"], layout, black, white, kind=case["kind"], tint=case["tint"])
        assert frame.dtype == np.uint16 and frame.shape == (case["h"], case["w"]) and int(frame.max()) < 1 << R.BITS[layout]
        assert np.array_equal(R.unpack(R.pack(frame, layout), case["w"], layout), frame)
    assert {c["layout"] for c in cases} == set(R.LAYOUTS) and {c["method"] for c in cases} == set(G.METHODS)
    assert {(c["layout"], c["method"]) for c in cases} == {(l, m) for l in R.LAYOUTS for m in G.METHODS}
    assert {c["flip"] for c in cases} == set(G.FLIPS) and {c["name"] for c in cases} == set(R.NAMES)
    assert {c["batch_layout"] for c in cases} == set(BATCH_LAYOUTS)
    assert {(c["layout"], c["path"]) for c in cases} == {(l, p) for l in R.LAYOUTS for p in ("interior", "byte")}
    assert {c["tap"] for c in cases} == {False, True} and any(c["range"] is None for c in cases) and any(c["range"] is not None for c in cases)


def test_sizes_cover_the_alignment_cases():
    for layout in R.LAYOUTS:
        s = PC.sizes(layout)
        assert all(w % R.WIDTH_MULTIPLE[layout] == 0 and w >= 3 for w, _ in s)
        assert {64, 128, 192, 196} <= {w for w, _ in s}
        assert any(-(-w // PC.TILE_W) >= 3 and -(-h // PC.TILE_H) >= 3 for w, h in s)
        assert any(PC.has_interior_tiles(w, h) for w, h in s)


# ---- C++ facade ---------------------------------------------------------------------------------------------------------------------
def build_cpp(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "packed_test.cpp")
    exe = str(tmp_path / "packed_test")
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-DRIP_NO_OPENCV", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
           "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_facade_packed_width_and_unpack(tmp_path, rip_lib):
    exe = build_cpp(tmp_path)
    env = dict(os.environ)
    env["RIP_DEVICE"] = "-1"
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "packed facade OK" in r.stdout


# ---- what the compiler made of the kernels -------------------------------------------------------------------------------------------
PACKED_SRC = os.path.join(ROOT, "raw_image_pipeline_amd", "csrc", "rip_packed.hip")


def test_packed_source_has_no_scratch_or_spills():
    """hipcc -Rpass-analysis=kernel-resource-usage on rip_packed.hip: 4 layouts x 2 methods x 4 patterns x 4 flips, no private
    segment, no spilled vector registers, the LDS of the uint16 kernel (the raw dwords wait in registers, not in LDS)."""
    from raw_image_pipeline_amd import build as B
    cmd = [B.hipcc()] + B.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-x", "hip", "-c", PACKED_SRC, "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    kernels = r.stderr.count("Function Name:")
    assert kernels == 128, kernels
    scratch = [l for l in r.stderr.splitlines() if "ScratchSize" in l]
    spills = [l for l in r.stderr.splitlines() if "Spill:" in l]
    assert len(scratch) == kernels and all(l.rstrip().endswith(" 0 [-Rpass-analysis=kernel-resource-usage]") for l in scratch), scratch
    # no register reaches memory.  (A few bilinear quarter-turn variants sit at the SGPR limit and park one or two scalar
    # registers in lanes of a vector register: that is no memory traffic and is not asserted on.)
    vspills = [l for l in spills if "VGPRs Spill" in l]
    assert len(vspills) == kernels and all(l.rstrip().endswith(" 0 [-Rpass-analysis=kernel-resource-usage]") for l in vspills), vspills
    lds = [int(l.split("LDS Size [bytes/block]:")[1].split()[0]) for l in r.stderr.splitlines() if "LDS Size" in l]
    assert len(lds) == kernels and max(lds) <= 5040 + 6144, lds


def test_packed_source_has_no_isa_hazards():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_hazard_check.py"), PACKED_SRC], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rip_packed.hip: 0 finding(s)" in r.stdout, r.stdout


def test_packed_source_is_compiled_into_the_library():
    from raw_image_pipeline_amd import build as B
    assert "rip_packed.hip" in B.SOURCES and "rip_raw16_dev.hpp" in B.HEADERS and "rip_unpack.hpp" in B.HEADERS
