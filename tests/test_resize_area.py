"""The resize stage under the "area" interpolation (include/rip.h rip_set_output_interpolation) without a GPU: the host-built tap
lists against tests/area_reference.py entry for entry, the reference against the known answers of PARITY.md "Resize: area
interpolation" and against the exact float64 box mean, the setter, the YAML key, geometry, camera matrices and refusals on
RIP_DEVICE_NONE handles, the C++ facade, and the kernels of csrc/rip_area.hip executed on the host against the reference."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import area_cases as AC
import area_reference as A
from helpers import CSRC, build_host_program
from raw_image_pipeline_amd import pipeline as P
from test_cpp_facade import BRANCHES, run_env
from test_resize import neutral, write_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = P.RIP_ERR_INVALID_ARGUMENT
LARGE_PAIRS = ((2448, 640), (2048, 480), (3840, 640), (16384, 64), (16384, 16383), (1001, 1000))


def hook(lib, R_, C_, H, W):
    xf, xc, xw = np.full(W, -7, np.int32), np.full(W, -7, np.int32), np.full(C_ + 2 * W, -7, np.float32)
    yf, yc, yw = np.full(H, -7, np.int32), np.full(H, -7, np.int32), np.full(R_ + 2 * H, -7, np.float32)
    whole, scale = C.c_int(-1), C.c_float(-1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    st = lib.rip_debug_resize_area_tables(R_, C_, H, W, ptr(xf), ptr(xc), ptr(xw), ptr(yf), ptr(yc), ptr(yw), C.byref(whole), C.byref(scale))
    return st, dict(xfirst=xf, xcount=xc, xweight=xw, yfirst=yf, ycount=yc, yweight=yw, whole=whole.value, scale=np.float32(scale.value))


def assert_tables(lib, R_, C_, H, W):
    st, got = hook(lib, R_, C_, H, W)
    assert st == P.RIP_OK, (R_, C_, H, W)
    want = A.tables(R_, C_, H, W)
    for axis in "xy":
        what = "%s axis of %d x %d -> %d x %d" % (axis, R_, C_, H, W)
        assert np.array_equal(got[axis + "first"], want[axis + "first"]) and np.array_equal(got[axis + "count"], want[axis + "count"]), what
        n = int(want[axis + "count"].sum())
        assert np.array_equal(got[axis + "weight"][:n].view(np.uint32), want[axis + "weight"].view(np.uint32)), what
        assert (got[axis + "weight"][n:] == -7).all(), what                                   # nothing written behind the last weight
    assert got["whole"] == want["whole"] and got["scale"].view(np.uint32) == np.float32(want["scale"]).view(np.uint32)


# ---- the tables ------------------------------------------------------------------------------------------------------------
def test_host_tables_equal_the_reference_for_every_downscale_pair_of_small_sides(rip_lib):
    for src in range(1, 41):
        for dst in range(1, src + 1):
            assert_tables(rip_lib, 7, src, 5, dst)
            assert_tables(rip_lib, src, 9, dst, 4)


@pytest.mark.parametrize("src,dst", LARGE_PAIRS)
def test_host_tables_equal_the_reference_for_large_sides(rip_lib, src, dst):
    assert_tables(rip_lib, 64, src, 7, dst)
    assert_tables(rip_lib, src, 64, dst, 7)


def axis_pairs():
    return [(s, d) for s in range(1, 41) for d in range(1, s + 1)] + list(LARGE_PAIRS)


def test_table_properties():
    """What the kernel relies on: every output has at least one tap, its taps are consecutive source samples inside the axis, and an
    axis holds at most s + 2 d of them.  Also: positive weights that sum to 1 within float rounding."""
    for s, d in axis_pairs():
        taps = A.axis_taps(s, d)
        assert len(taps) == d
        total = 0
        for tp in taps:
            idx = [k for k, _ in tp]
            assert len(idx) >= 1 and idx == list(range(idx[0], idx[0] + len(idx))) and idx[0] >= 0 and idx[-1] < s, (s, d, idx)
            assert all(w > 0 for _, w in tp) and abs(sum(float(w) for _, w in tp) - 1.0) < 2e-3, (s, d, tp)
            total += len(idx)
        assert total <= s + 2 * d, (s, d, total)
        first = [tp[0][0] for tp in taps]
        assert first == sorted(first) and first[0] == 0 and taps[-1][-1][0] == s - 1, (s, d)


def test_the_whole_flag_and_scale(rip_lib):
    for (R_, C_, H, W), whole in (((8, 12, 2, 3), True), ((8, 12, 4, 6), False), ((8, 12, 8, 12), False), ((8, 12, 8, 4), True), ((8, 12, 4, 12), True),
                                  ((8, 12, 2, 5), False), ((8, 12, 3, 3), False), ((512, 256, 2, 1), True)):
        st, t = hook(rip_lib, R_, C_, H, W)
        assert st == P.RIP_OK and t["whole"] == int(whole), (R_, C_, H, W)
        assert t["scale"] == (np.float32(1) / np.float32((R_ // H) * (C_ // W)) if whole else 0)


def test_the_hook_refuses_bad_sizes_upscales_large_factors_and_null_tables(rip_lib):
    i32, f32 = np.full(600, -7, np.int32), np.full(2000, -7, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for bad in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (-1, 4, 4, 4), (16385, 4, 4, 4), (4, 4, 5, 4), (4, 4, 4, 5), (4, 257, 4, 1), (513, 4, 2, 4)):
        assert rip_lib.rip_debug_resize_area_tables(*bad, ptr(i32), ptr(i32), ptr(f32), ptr(i32), ptr(i32), ptr(f32), None, None) == INVALID, bad
        assert (i32 == -7).all() and (f32 == -7).all()
    assert rip_lib.rip_debug_resize_area_tables(4, 256, 4, 1, ptr(i32), ptr(i32), ptr(f32), ptr(i32), ptr(i32), ptr(f32), None, None) == P.RIP_OK
    assert rip_lib.rip_debug_resize_area_tables(4, 4, 2, 2, None, ptr(i32), ptr(f32), ptr(i32), ptr(i32), ptr(f32), None, None) == INVALID


# ---- known answers and the independent bound -----------------------------------------------------------------------------------
def test_known_answers():
    f32 = lambda v: np.float32(v)
    assert A.axis_taps(3, 2) == [[(0, f32(2 / 3)), (1, f32(1 / 3))], [(1, f32(1 / 3)), (2, f32(2 / 3))]]
    assert A.resize(np.array([[0, 90, 255]], np.uint8), 1, 2).tolist() == [[30, 200]]
    for total, want in ((8, 0), (24, 2), (40, 2)):                                   # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2: half to even
        block = np.zeros(16, np.uint8)
        block[:total // 8] = 8
        assert int(block.sum()) == total and A.resize(block.reshape(4, 4), 1, 1).tolist() == [[want]]
    assert A.resize(np.array([[1, 0], [1, 0]], np.uint8), 1, 1).tolist() == [[1]]    # the 2 x 2 rule: (2 + 2) >> 2, half up
    t = A.axis_taps(6, 5)
    assert t[0] == [(0, f32(0.8333333)), (1, f32(0.16666667))] and t[-1] == [(4, f32(0.16666667)), (5, f32(0.8333333))]
    assert A.axis_taps(5, 5) == [[(i, f32(1))] for i in range(5)]
    ties = A.resize(AC.tie_frame(1), 2, 6)
    assert ties.tolist() == [[0, 2, 2, 4, 4, 6], [0, 1, 1, 2, 252, 252]]


BOUND_SIZES = (((10, 15), (4, 6)), ((7, 9), (7, 4)), ((33, 65), (13, 17)), ((48, 64), (12, 32)), ((9, 9), (8, 8)), ((20, 30), (3, 7)), ((40, 40), (1, 1)),
               ((17, 23), (5, 23)), ((30, 50), (29, 49)), ((5, 1001), (5, 1000)))


@pytest.mark.parametrize("src,dst", BOUND_SIZES)
def test_the_reference_stays_within_one_lsb_of_the_exact_box_mean(src, dst):
    """(rows, cols) -> (rows, cols) on seeded random frames, both channel counts.  The taps drop slivers below 1e-3 of a pixel and
    renormalise, and the result is rounded: measured at most 0.5 on all of these, the bound is 1.0.  Flat 255 stays flat 255."""
    rng = np.random.default_rng(11)
    for cn in (1, 3):
        f = rng.integers(0, 256, src if cn == 1 else src + (3,), dtype=np.uint8)
        got, exact = A.resize(f, *dst), A.box_mean(f, *dst)
        err = float(np.abs(got.astype(np.float64) - exact).max())
        print("%s -> %s x %d: max |reference - box mean| = %.4f" % (src, dst, cn, err))
        assert got.shape == exact.shape and err <= 1.0
        flat = np.full_like(f, 255)
        assert (A.resize(flat, *dst) == 255).all()


# ---- the parameter surface -------------------------------------------------------------------------------------------------
def test_defaults_set_get_and_reject(host_pipe):
    p = host_pipe
    assert p.get_output_interpolation() == "linear"
    for name in ("area", "linear", "area"):
        p.set_output_interpolation(name)
        assert p.get_output_interpolation() == name
    for bad in ("", "Area", "AREA", "cubic", "nearest", "area ", "lanczos"):
        with pytest.raises(ValueError) as e:
            p.set_output_interpolation(bad)
        assert '"linear" or "area"' in str(e.value)
        assert p.get_output_interpolation() == "area"
    lib = p._lib
    assert lib.rip_set_output_interpolation(None, b"area") == INVALID and lib.rip_set_output_interpolation(p._h, None) == INVALID
    assert p.get_output_interpolation() == "area"
    buf = C.create_string_buffer(2)
    assert lib.rip_get_output_interpolation(p._h, buf, C.c_size_t(2)) != P.RIP_OK          # no room for the name
    assert p.get_output_size() == (0, 0)                                                      # the setting alone activates nothing
    assert p.query_output(30, 44, 3, "bgr8") == (30, 44, 3, "bgr8")


def test_yaml_key(tmp_path, host_pipe):
    p = host_pipe
    p.load_params(write_params(tmp_path, "output:\n  size: [640, 512]\n  interpolation: area\n"))
    assert p.get_output_interpolation() == "area" and p.get_output_size() == (640, 512)
    p.load_params(write_params(tmp_path, "output:\n  size: [640, 512]\n"))                    # absent: linear
    assert p.get_output_interpolation() == "linear"
    p.set_output_interpolation("area")
    p.load_params(write_params(tmp_path, "output:\n  interpolation: linear\n"))
    assert p.get_output_interpolation() == "linear"
    p.set_output_interpolation("area")
    p.load_params(write_params(tmp_path, "debayer:\n  enabled: true\n"))                      # rip_load_params re-creates the modules
    assert p.get_output_interpolation() == "linear"


@pytest.mark.parametrize("bad", ["cubic", "Area", "1", "[area]", "''"])
def test_yaml_invalid_value_fails_and_changes_nothing(tmp_path, host_pipe, bad):
    p = host_pipe
    p.set_output_size(33, 17)
    p.set_output_interpolation("area")
    p.set_output_format("bgr_chw_f32")
    p.set_flip(True)
    p.set_flip_angle(180)
    with pytest.raises(ValueError):
        p.load_params(write_params(tmp_path, "output:\n  size: [8, 8]\n  interpolation: %s\n  format: rgb8\nflip:\n  enabled: false\n" % bad))
    assert p.get_output_interpolation() == "area" and p.get_output_size() == (33, 17) and p.get_output_format() == "bgr_chw_f32" and p.is_flip_enabled()


# ---- geometry, camera matrices, refusals ------------------------------------------------------------------------------------
CALLS = ("query_output", "query_output_bytes", "get_output_camera_info")


def test_geometry_and_camera_matrices_equal_the_linear_ones(host_pipe):
    from raw_image_pipeline_amd import synth
    p = host_pipe
    neutral(p)
    synth.load_camera(p, synth.camera_model(64, 48))
    for fmt in ("native", "rgb8", "mono8", "rgb_chw_f16", "bgr_chw_f32"):
        p.set_output_format(fmt)
        for target in ((0, 0), (64, 48), (32, 24), (16, 12), (17, 9), (64, 9), (1, 1), (21, 48)):
            p.set_output_size(*target)
            answers = {}
            for name in ("linear", "area"):
                p.set_output_interpolation(name)
                q = p.get_output_camera_info(48, 64, 1, "bayer_rggb8")
                answers[name] = (p.query_output(48, 64, 1, "bayer_rggb8"), p.query_output_bytes(48, 64, 1, "bayer_rggb8"), p.query_taps(48, 64, 1, "bayer_rggb8"),
                                 q[:2], q[2].tobytes(), q[3].tobytes())
            assert answers["linear"] == answers["area"], (fmt, target)
            if target != (0, 0):
                assert answers["area"][0][:2] == (target[1], target[0])
    p.set_flip(True)                                  # a flip by 90 degrees swaps the sides the rules look at
    p.set_flip_angle(90)
    p.set_output_format("native")
    p.set_output_interpolation("area")
    p.set_output_size(48, 64)
    assert p.query_output(48, 64, 1, "bayer_rggb8")[:2] == (64, 48)
    p.set_output_size(49, 64)
    with pytest.raises(ValueError):
        p.query_output(48, 64, 1, "bayer_rggb8")


def test_refusals(host_pipe):
    p = host_pipe
    neutral(p)
    p.set_output_interpolation("area")
    for target, word in (((45, 30), "downscale"), ((44, 31), "downscale"), ((88, 60), "downscale"), ((45, 10), "downscale")):   # (a): W > C or H > R
        p.set_output_size(*target)
        for call in CALLS:
            with pytest.raises(ValueError) as e:
                getattr(p, call)(30, 44, 3, "bgr8")
            assert word in str(e.value), (target, call)
        p.set_output_interpolation("linear")
        assert p.query_output(30, 44, 3, "bgr8")[:2] == (target[1], target[0])        # the linear filter takes them all
        p.set_output_interpolation("area")
    # (b): C > 256 W or R > 256 H; exactly 256 is accepted
    p.set_output_size(2, 3)
    assert p.query_output(768, 512, 1, "mono8")[:2] == (3, 2)
    for rows, cols in ((768, 513), (769, 512)):
        for call in CALLS:
            with pytest.raises(ValueError) as e:
                getattr(p, call)(rows, cols, 1, "mono8")
            assert "256" in str(e.value)
    p.set_output_size(1, 1)
    assert p.query_output(256, 256, 1, "mono8")[:2] == (1, 1)
    with pytest.raises(ValueError):
        p.query_output(257, 1, 1, "mono8")
    # the existing refusals still apply under area
    p.set_output_size(64, 64)
    with pytest.raises(ValueError) as e:
        p.query_output(64, 16385, 1, "mono8")
    assert "16384" in str(e.value)
    assert p.query_output(64, 16384, 1, "mono8")[:2] == (64, 64)
    p.set_debayer_16bit(True)
    p.set_output_size(17, 9)
    with pytest.raises(ValueError) as e:
        p.query_output(30, 44, 1, "bayer_rggb16")
    assert "bgr16" in str(e.value)
    # F's own size and no target: nothing to refuse
    p.set_debayer_16bit(False)
    p.set_output_size(44, 30)
    assert p.query_output(30, 44, 3, "bgr8") == (30, 44, 3, "bgr8")
    p.set_output_size(0, 0)
    assert p.query_output(30, 44, 3, "bgr8") == (30, 44, 3, "bgr8")


def test_frame_calls_need_a_device_under_area_too(host_pipe):
    host_pipe.set_output_size(4, 4)
    host_pipe.set_output_interpolation("area")
    with pytest.raises(P.RipError):
        host_pipe.process(np.zeros((8, 8), np.uint8), "bayer_rggb8")


# ---- C++ facade ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade_sets_gets_and_throws(tmp_path, rip_lib, branch):
    exe = str(tmp_path / ("area_test_" + branch.replace("-", "_")))
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror"] + BRANCHES[branch] + ["-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "area_test.cpp"), "-o", exe, "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir,
           "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=run_env(-1))
    assert r.returncode == 0 and "area host OK" in r.stdout, r.stdout + r.stderr


# ---- the kernels, executed on the host -----------------------------------------------------------------------------------------
def host_cases():
    """(R, C, H, W, channels, frames, row padding, offset, frame gap, frames' pixels) of every case the GPU tests run through the area
    kernels: the shapes of tests/area_cases.py under both channel counts and three destination layouts, the crafted frames, and the
    fuzz draws."""
    out = []
    rng = np.random.default_rng(23)

    def add(src, dst, cn, n, pad, off, gap, frames=None):
        (sw, sh), (dw, dh) = src, dst
        if frames is None:
            frames = rng.integers(0, 256, (n, sh, sw, cn), dtype=np.uint8)
        out.append((sh, sw, dh, dw, cn, n, pad, off, gap, np.ascontiguousarray(frames).reshape(n, sh, sw, cn)))
    for s in AC.SHAPES:
        if s.kind == "mean2":
            continue
        for cn in (1, 3):
            for pad, off, gap in ((0, 0, 0), (5, 1, 3), (16, 3, 0)):
                add(s.src, s.dst, cn, 2, pad, off, gap)
    for cn in (1, 3):
        add((24, 8), (6, 2), cn, 1, 0, 0, 0, AC.tie_frame(cn)[None])
        add((512, 256), (2, 1), cn, 1, 0, 0, 0, AC.all_255((512, 256), cn)[None])
        add((153, 128), (40, 30), cn, 1, 0, 0, 0, AC.all_255((153, 128), cn)[None])
    for seed in range(AC.FUZZ_CASES):
        k = AC.fuzz_case(seed)
        if AC.kind_of(k["src"], k["dst"]) in ("general", "whole"):
            add(k["src"], k["dst"], k["cn"], k["n"], (0, 1, 16)[k["pitch"]], int(k["base_off"]), 5 if k["gap"] else 0)
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_kernels_run_on_the_host_equal_the_reference_byte_for_byte(tmp_path, rip_lib, sanitize):
    """tests/cpp/area_kernel_host.cpp: csrc/rip_area.hip compiled as host code with the toolchain's clang++ (-ffp-contract=off), every
    thread of the launcher's grid run in turn into exactly sized buffers with sentinels, tables in exactly sized heap blocks.
    The second build adds -fsanitize=address,undefined to this stand-alone program (no out-of-bounds access, no
    misaligned wide access)."""
    exe = build_host_program(tmp_path, "area_kernel_host", ["area_kernel_host.cpp", os.path.join(CSRC, "rip_output_tables.cpp")], sanitize=sanitize,
                             extra=["-ffp-contract=off", "-lm", "-lpthread"])
    cases = host_cases()
    assert len(cases) >= 100
    cases_path, out_path = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(cases_path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            f.write(struct.pack("<9i", *c[:9]))
            f.write(c[9].tobytes())
    r = subprocess.run([exe, cases_path, out_path], capture_output=True, text=True)
    assert r.returncode == 0 and "%d cases, 0 bad" % len(cases) in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.fromfile(out_path, np.uint8)
    at = 0
    for (R_, C_, H, W, cn, n, pad, off, gap, frames) in cases:
        step = W * cn + pad
        frame = step * H + gap
        total = off + frame * (n - 1) + step * (H - 1) + W * cn
        want = np.full(total, 0xA5, np.uint8)
        for k in range(n):
            small = A.resize(frames[k] if cn == 3 else frames[k, :, :, 0], H, W).reshape(H, W * cn)
            for y in range(H):
                o = off + k * frame + y * step
                want[o:o + W * cn] = small[y]
        what = "%d x %d x %d -> %d x %d, %d frames, pad %d off %d gap %d" % (C_, R_, cn, W, H, n, pad, off, gap)
        assert np.array_equal(got[at:at + total], want), "%s: %d bytes differ" % (what, int((got[at:at + total] != want).sum()))
        at += total
    assert at == got.size
