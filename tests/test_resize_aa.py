"""The resize stage under "linear_aa" and "cubic_aa" (include/rip.h rip_set_output_interpolation) without a GPU: tests/aa_reference.py
pinned to torch.nn.functional.interpolate(uint8, antialias=True) byte for byte, the host-built tables against the reference entry for
entry, known answers worked by hand, the setter, the YAML key, geometry, camera matrices and refusals on RIP_DEVICE_NONE handles,
the C++ facade, and the kernels of csrc/rip_aa.hip executed on the host against the reference."""
import ctypes as C
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import aa_cases as AC
import aa_reference as A
from helpers import CSRC, build_host_program
from raw_image_pipeline_amd import pipeline as P
from test_cpp_facade import BRANCHES, run_env
from test_resize import neutral, write_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = P.RIP_ERR_INVALID_ARGUMENT
LARGE_PAIRS = ((2448, 640), (2048, 480), (4096, 64), (16384, 256), (16383, 16384), (1000, 1001))
NAMES = AC.FILTER_NAMES


# ---- the pin: the reference equals torch ----------------------------------------------------------------------------------------------
def test_the_reference_equals_torch_interpolate_byte_for_byte():
    """578 cases per filter: 558 seeded draws with sides in 1..200 (upscales, one axis unchanged, 1 and 3 channels, random and 0 / 255
    images, contiguous and channels_last) and the fixed pairs of tests/aa_cases.py.  Only targets of exactly 1 x 1 are left out (torch
    asserts there).  torch's vectorised uint8 path is the definition: other CPUs take another path, so the test is skipped there."""
    import torch
    capability = torch.backends.cpu.get_cpu_capability()
    if capability not in ("AVX2", "AVX512"):
        pytest.skip("torch's antialiased uint8 path is the AVX2 / AVX512 one; this CPU gives %s" % capability)
    cases = AC.pin_cases()
    assert len(cases) == 578 and all(c.dst != (1, 1) and c.channels <= 4 for c in cases)
    assert {c.channels for c in cases} == {1, 3} and {c.binary for c in cases} == {False, True} and {c.channels_last for c in cases} == {False, True}
    assert any(c.dst[0] > c.src[0] for c in cases) and any(c.dst[0] == c.src[0] and c.dst[1] != c.src[1] for c in cases)
    rng = np.random.default_rng(31)
    worst = 0
    for k, c in enumerate(cases):
        (sw, sh), (dw, dh) = c.src, c.dst
        img = rng.integers(0, 2, (sh, sw, c.channels), dtype=np.uint8) * 255 if c.binary else rng.integers(0, 256, (sh, sw, c.channels), dtype=np.uint8)
        for name in NAMES:
            want = A.torch_resize(img, dh, dw, name, c.channels_last)
            got = A.resize(img, dh, dw, name)
            diff = int(np.abs(got.astype(np.int32) - want).max())
            worst = max(worst, diff)
            assert diff == 0, "case %d %s %s: max |reference - torch| = %d" % (k, c, name, diff)
    print("max |reference - torch| over %d cases x 2 filters: %d" % (len(cases), worst))


# ---- the tables ------------------------------------------------------------------------------------------------------------------------
def hook(lib, name, R_, C_, H, W, cn=3):
    S = A.FILTERS[name][1]
    cap = lambda s, d: 2 * S * max(s, d) + d
    i32 = lambda n: np.full(n, -7, np.int32)
    t = dict(xfirst=i32(W), xcount=i32(W), xwofs=i32(W), xweight=np.full(cap(C_, W), -7, np.int16), yfirst=i32(H), ycount=i32(H), ywofs=i32(H),
             yweight=np.full(cap(R_, H), -7, np.int16))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ints = [C.c_int(-1) for _ in range(4)]
    st = lib.rip_debug_resize_aa_tables(name.encode(), R_, C_, H, W, cn, ptr(t["xfirst"]), ptr(t["xcount"]), ptr(t["xwofs"]), ptr(t["xweight"]), ptr(t["yfirst"]),
                                        ptr(t["ycount"]), ptr(t["ywofs"]), ptr(t["yweight"]), *[C.byref(v) for v in ints])
    t.update(xprec=ints[0].value, yprec=ints[1].value, tile_rows=ints[2].value, lds_rows=ints[3].value)
    return st, t


def assert_tables(lib, name, R_, C_, H, W):
    st, got = hook(lib, name, R_, C_, H, W)
    assert st == P.RIP_OK, (name, R_, C_, H, W)
    for ax, s, d in (("x", C_, W), ("y", R_, H)):
        want = A.axis(name, s, d)
        what = "%s: %s axis of %d x %d -> %d x %d" % (name, ax, R_, C_, H, W)
        for part in ("first", "count", "wofs"):
            assert np.array_equal(got[ax + part], want[part]), (what, part)
        n = len(want["weight"])
        assert np.array_equal(got[ax + "weight"][:n], want["weight"]), what
        assert (got[ax + "weight"][n:] == -7).all(), what                                   # nothing written behind the last weight
        assert got[ax + "prec"] == want["prec"], what
    for cn in (1, 3):
        st, got = hook(lib, name, R_, C_, H, W, cn)
        assert (got["tile_rows"], got["lds_rows"]) == A.tile_rows(name, R_, H, cn), (name, R_, H, cn)


@pytest.mark.parametrize("name", NAMES)
def test_host_tables_equal_the_reference_for_every_pair_of_small_sides(rip_lib, name):
    for src in range(1, 41):
        for dst in range(1, 41):
            assert_tables(rip_lib, name, 7, src, 5, dst)
            assert_tables(rip_lib, name, src, 9, dst, 4)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("src,dst", LARGE_PAIRS)
def test_host_tables_equal_the_reference_for_large_sides(rip_lib, name, src, dst):
    assert_tables(rip_lib, name, 64, src, 7, dst)
    assert_tables(rip_lib, name, src, 64, dst, 7)


def test_table_properties():
    """What the kernel relies on: every output has at least one tap, its taps lie inside [0, s), first and first + count do not
    decrease along the axis (a tile's rows read one span), an axis holds at most 2 S max(s, d) + d weights, the weights of an output
    sum to 2^prec within the rounding of its taps (half a unit each), and 255 * sum |q| stays below 2^31."""
    pairs = [(s, d) for s in range(1, 41) for d in range(1, 41)] + list(LARGE_PAIRS) + [(1280, 20), (16384, 256), (64, 1), (128, 2)]
    for name in NAMES:
        S = A.FILTERS[name][1]
        for s, d in pairs:
            t = A.axis(name, s, d)
            first, count = t["first"].astype(np.int64), t["count"].astype(np.int64)
            assert len(first) == d and (count >= 1).all() and (first >= 0).all() and (first + count <= s).all(), (name, s, d)
            assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all(), (name, s, d)
            assert len(t["weight"]) == count.sum() <= 2 * S * max(s, d) + d, (name, s, d)
            assert 1 <= t["prec"] <= 22
            for i in range(d):
                q = t["weight"][t["wofs"][i]:t["wofs"][i] + count[i]].astype(np.int64)
                assert abs(int(q.sum()) - (1 << t["prec"])) <= 0.5 * count[i] + 1e-6 * (1 << t["prec"]), (name, s, d, i)
                assert 255 * int(np.abs(q).sum()) < 2 ** 31, (name, s, d, i)
            if s == d:                                  # the skipped pass would be the identity
                x = np.arange(s, dtype=np.uint8)[None, :, None] * 3
                assert np.array_equal(A.one_pass(x, t), x)


def test_the_tile_height_is_the_largest_that_fits_64_kib(rip_lib):
    seen = set()
    for name, cn, (sw, sh), (dw, dh) in AC.TILE_HEIGHT_SHAPES:
        st, t = hook(rip_lib, name, sh, sw, dh, dw, cn)
        assert st == P.RIP_OK
        th, rows = t["tile_rows"], t["lds_rows"]
        assert (th, rows) == A.tile_rows(name, sh, dh, cn) and rows * 64 * cn <= 65536
        if th < 8:                                      # twice the height would not fit
            first, count = A.axis(name, sh, dh)["first"], A.axis(name, sh, dh)["count"]
            spans = [int(first[min(dh, y + 2 * th) - 1] + count[min(dh, y + 2 * th) - 1] - first[y]) for y in range(0, dh, 2 * th)]
            assert max(spans) * 64 * cn > 65536
        seen.add(th)
    # a cubic output row at a factor of 64 reads 257 source rows and two read 321: 61 632 bytes with 3 channels, so a height of 1 is
    # never the choice under the factor cap -- it stays the kernel's floor and runs in the host-run test below
    assert seen == {8, 4, 2}
    assert hook(rip_lib, "cubic_aa", 1280, 8, 20, 8, 3)[1]["tile_rows"] == 2


def test_the_hook_refuses_bad_sizes_large_factors_other_names_and_null_tables(rip_lib):
    i32, i16 = np.full(4000, -7, np.int32), np.full(8000, -7, np.int16)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda name, sizes, cn=3, first=ptr(i32): rip_lib.rip_debug_resize_aa_tables(name, *sizes, cn, first, ptr(i32), None, ptr(i16), ptr(i32), ptr(i32), None,
                                                                                        ptr(i16), None, None, None, None)
    for bad in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (-1, 4, 4, 4), (16385, 4, 4, 4), (4, 65, 4, 1), (129, 4, 2, 4)):
        assert call(b"cubic_aa", bad) == INVALID, bad
        assert (i32 == -7).all() and (i16 == -7).all()
    assert call(b"cubic_aa", (4, 64, 4, 1)) == P.RIP_OK and call(b"linear_aa", (128, 4, 2, 9)) == P.RIP_OK
    for name in (b"linear", b"area", b"cubic", b"", None):
        assert call(name, (4, 4, 2, 2)) == INVALID
    assert call(b"linear_aa", (4, 4, 2, 2), cn=2) == INVALID
    assert call(b"linear_aa", (4, 4, 2, 2), first=None) == INVALID


# ---- known answers, worked by hand ---------------------------------------------------------------------------------------------------
def test_known_answers():
    """3 -> 2: scale 1.5, centres 0.75 and 2.25.  linear_aa: support 1.5, taps at t = -1/6, 1/2 -> 5/6, 1/2 -> normalised 5/8, 3/8; the
    largest weight 5/8 gives prec 15.  cubic_aa: support 3, all three samples, t = -1/6, 1/2, 7/6 -> 15/16, 9/16, -25/432 -> normalised
    405/623, 243/623, -25/623.  2 -> 4: scale 1/2, the filters unstretched, centres 0.25, 0.75, ...: linear_aa gives [a, (3a + b)/4,
    (a + 3b)/4, b] with prec 14; cubic_aa gives the outer pixels k(1/4), k(5/4) = 111/128, -9/128 -> 37/34, -3/34 and the inner ones
    k(1/4), k(3/4) = 111/128, 29/128 -> 111/140, 29/140."""
    def weights(name, s, d):
        t = A.axis(name, s, d)
        return [[Fraction(float(v)).limit_denominator(10000) for v in t["w"][o:o + n]] for o, n in zip(t["wofs"], t["count"])], t
    F_ = Fraction
    w, t = weights("linear_aa", 3, 2)
    assert w == [[F_(5, 8), F_(3, 8)], [F_(3, 8), F_(5, 8)]] and t["first"].tolist() == [0, 1] and t["prec"] == 15
    assert t["weight"].tolist() == [20480, 12288, 12288, 20480]
    assert A.resize(np.array([[0, 90, 255]], np.uint8), 1, 2, "linear_aa").tolist() == [[34, 193]]           # 33.75, 193.125
    w, t = weights("cubic_aa", 3, 2)
    assert w == [[F_(405, 623), F_(243, 623), F_(-25, 623)], [F_(-25, 623), F_(243, 623), F_(405, 623)]] and t["first"].tolist() == [0, 0]
    assert t["prec"] == 15 and t["weight"].tolist() == [21302, 12781, -1315, -1315, 12781, 21302]          # 21301.8, 12781.1, -1314.9
    assert A.resize(np.array([[0, 90, 255]], np.uint8), 1, 2, "cubic_aa").tolist() == [[25, 201]]            # (90 * 243 - 255 * 25) / 623 = 24.87; 200.87
    w, t = weights("linear_aa", 2, 4)
    assert w == [[F_(1)], [F_(3, 4), F_(1, 4)], [F_(1, 4), F_(3, 4)], [F_(1)]] and t["first"].tolist() == [0, 0, 0, 1] and t["prec"] == 14
    assert A.resize(np.array([[0, 200]], np.uint8), 1, 4, "linear_aa").tolist() == [[0, 50, 150, 200]]
    w, t = weights("cubic_aa", 2, 4)
    assert w == [[F_(37, 34), F_(-3, 34)], [F_(111, 140), F_(29, 140)], [F_(29, 140), F_(111, 140)], [F_(-3, 34), F_(37, 34)]]
    unclipped = []
    assert A.resize(np.array([[0, 200]], np.uint8), 1, 4, "cubic_aa", unclipped).tolist() == [[0, 41, 159, 218]]   # -17.6 clamped; 41.4, 158.6, 217.6
    assert unclipped == [(-18, 255)]
    assert A.resize(np.array([[255, 0]], np.uint8), 1, 4, "cubic_aa").tolist() == [[255, 202, 53, 0]]        # 277.5 clamped; 202.2, 52.8, -22.5
    # exactly half: torch's taps 1/8, 3/8, 3/8, 1/8, not the block mean
    t = A.axis("linear_aa", 8, 4)
    assert [Fraction(float(v)).limit_denominator(100) for v in t["w"][t["wofs"][1]:t["wofs"][1] + 4]] == [F_(1, 8), F_(3, 8), F_(3, 8), F_(1, 8)]
    # the vertical pass works on the rounded horizontal pass
    img = np.array([[0, 90, 255], [255, 90, 0], [10, 20, 30]], np.uint8)
    h = np.stack([A.resize(r[None], 1, 2, "linear_aa")[0] for r in img])
    assert h.tolist() == [[34, 193], [193, 34], [14, 26]]                                                      # 13.75, 26.25
    assert A.resize(img, 2, 2, "linear_aa").tolist() == [[94, 133], [81, 29]]   # (5 * 34 + 3 * 193) / 8 = 93.6; 133.4; (3 * 193 + 5 * 14) / 8 = 81.1; 29


# ---- the parameter surface -------------------------------------------------------------------------------------------------------------
def test_defaults_set_get_and_reject(host_pipe):
    p = host_pipe
    assert p.get_output_interpolation() == "linear"
    for name in ("linear_aa", "cubic_aa", "linear", "area", "cubic_aa"):
        p.set_output_interpolation(name)
        assert p.get_output_interpolation() == name
    for bad in ("", "cubic", "nearest", "lanczos", "Linear_aa", "CUBIC_AA", "cubic_aa ", "bicubic", "linear-aa"):
        with pytest.raises(ValueError) as e:
            p.set_output_interpolation(bad)
        assert '"linear" or "area"' in str(e.value) and '"linear_aa" or "cubic_aa"' in str(e.value)
        assert p.get_output_interpolation() == "cubic_aa"
    assert p._lib.rip_set_output_interpolation(p._h, None) == INVALID and p.get_output_interpolation() == "cubic_aa"
    assert p.get_output_size() == (0, 0)                                                      # the setting alone activates nothing
    assert p.query_output(30, 44, 3, "bgr8") == (30, 44, 3, "bgr8")


@pytest.mark.parametrize("name", NAMES)
def test_yaml_key(tmp_path, host_pipe, name):
    p = host_pipe
    p.load_params(write_params(tmp_path, "output:\n  size: [640, 480]\n  interpolation: %s\n" % name))
    assert p.get_output_interpolation() == name and p.get_output_size() == (640, 480)
    p.load_params(write_params(tmp_path, "output:\n  size: [640, 480]\n"))                    # absent: linear
    assert p.get_output_interpolation() == "linear"


@pytest.mark.parametrize("bad", ["cubic", "nearest", "lanczos", "Cubic_aa", "[cubic_aa]"])
def test_yaml_invalid_value_fails_and_changes_nothing(tmp_path, host_pipe, bad):
    p = host_pipe
    p.set_output_size(33, 17)
    p.set_output_interpolation("linear_aa")
    with pytest.raises(ValueError) as e:
        p.load_params(write_params(tmp_path, "output:\n  size: [8, 8]\n  interpolation: %s\n" % bad))
    assert '"linear" or "area"' in str(e.value)
    assert p.get_output_interpolation() == "linear_aa" and p.get_output_size() == (33, 17)


# ---- geometry, camera matrices, refusals ---------------------------------------------------------------------------------------------
CALLS = ("query_output", "query_output_bytes", "get_output_camera_info", "get_output_window")


def test_geometry_and_camera_matrices_equal_the_linear_ones(host_pipe):
    from raw_image_pipeline_amd import synth
    p = host_pipe
    neutral(p)
    synth.load_camera(p, synth.camera_model(64, 48))
    for fmt in ("native", "rgb8", "mono8", "rgb_chw_f16"):
        p.set_output_format(fmt)
        for fit, roi in (("stretch", (0, 0, 0, 0)), ("letterbox", (0, 0, 0, 0)), ("crop", (3, 5, 40, 30))):
            p.set_output_fit(fit)
            p.set_output_roi(*roi)
            for target in ((0, 0), (64, 48), (32, 24), (17, 9), (64, 9), (1, 1), (100, 90), (21, 48)):
                p.set_output_size(*target)
                answers = {}
                for name in ("linear",) + NAMES:
                    p.set_output_interpolation(name)
                    q = p.get_output_camera_info(48, 64, 1, "bayer_rggb8")
                    answers[name] = (p.query_output(48, 64, 1, "bayer_rggb8"), p.query_output_bytes(48, 64, 1, "bayer_rggb8"), p.query_taps(48, 64, 1, "bayer_rggb8"),
                                     p.get_output_window(48, 64, 1, "bayer_rggb8"), q[:2], q[2].tobytes(), q[3].tobytes())
                assert answers["linear"] == answers["linear_aa"] == answers["cubic_aa"], (fmt, fit, target)


@pytest.mark.parametrize("name", NAMES)
def test_the_factor_64_refusal_and_its_place_in_the_order(host_pipe, name):
    p = host_pipe
    neutral(p)
    p.set_output_interpolation(name)
    # exactly 64 on both axes is accepted, 64 and a pixel on either axis is refused; upscales are accepted
    p.set_output_size(2, 3)
    assert p.query_output(192, 128, 1, "mono8")[:2] == (3, 2)
    for rows, cols in ((192, 129), (193, 128)):
        for call in CALLS:
            with pytest.raises(ValueError) as e:
                getattr(p, call)(rows, cols, 1, "mono8")
            assert "64 per axis" in str(e.value), call
    p.set_output_size(16384, 16384)
    assert p.query_output(5, 7, 3, "bgr8")[:2] == (16384, 16384)
    p.set_output_interpolation("linear")                       # the other filters keep their own rules
    p.set_output_size(2, 3)
    assert p.query_output(193, 129, 1, "mono8")[:2] == (3, 2)
    p.set_output_interpolation(name)
    # after a bgr16 result
    p.set_debayer_16bit(True)
    with pytest.raises(ValueError) as e:
        p.query_output(200, 200, 1, "bayer_rggb16")
    assert "bgr16" in str(e.value)
    p.set_debayer_16bit(False)
    # after a side of F above 16384 (here the factor is beyond 64 too)
    with pytest.raises(ValueError) as e:
        p.query_output(64, 16385, 1, "mono8")
    assert "larger than" in str(e.value)
    # after the window outside F; and the rule looks at the window, not at F
    p.set_output_roi(0, 0, 130, 10)
    with pytest.raises(ValueError) as e:
        p.query_output(100, 100, 1, "mono8")
    assert "does not lie inside" in str(e.value)
    p.set_output_size(2, 10)
    with pytest.raises(ValueError) as e:
        p.query_output(100, 200, 1, "mono8")
    assert "64 per axis" in str(e.value)
    p.set_output_roi(5, 7, 128, 10)
    assert p.query_output(100, 200, 1, "mono8")[:2] == (10, 2)
    # window size == picture size: the copy, nothing to refuse; F's own size and no target: nothing at all
    p.set_output_roi(0, 0, 0, 0)
    p.set_output_size(44, 30)
    assert p.query_output(30, 44, 3, "bgr8") == (30, 44, 3, "bgr8")
    p.set_output_size(0, 0)
    assert p.query_output(3000, 44, 3, "bgr8") == (3000, 44, 3, "bgr8")


def test_frame_calls_need_a_device_under_the_antialiased_filters_too(host_pipe):
    host_pipe.set_output_size(4, 4)
    host_pipe.set_output_interpolation("cubic_aa")
    with pytest.raises(P.RipError):
        host_pipe.process(np.zeros((8, 8), np.uint8), "bayer_rggb8")


# ---- C++ facade --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade_sets_gets_and_throws(tmp_path, rip_lib, branch):
    exe = str(tmp_path / ("aa_test_" + branch.replace("-", "_")))
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror"] + BRANCHES[branch] + ["-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "aa_test.cpp"), "-o", exe, "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir,
           "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=run_env(-1))
    assert r.returncode == 0 and "aa host OK" in r.stdout, r.stdout + r.stderr


# ---- the kernels, executed on the host -----------------------------------------------------------------------------------------------
FILTER_ID = {"linear_aa": 2, "cubic_aa": 3}
WINDOW_ORIGINS = ((0, 0), (1, 2), (2, 1), (3, 3), (5, 0))     # every byte phase of the first column, for 1 and for 3 channels


def host_cases():
    """(filter, R, C of F, window x, y, w, h, H, W, channels, frames, row padding, offset, frame gap, forced tile height, F's pixels) of
    every shape the GPU tests run: tests/aa_cases.py SHAPES under both filters, both channel counts and both kernels (all of F; a
    window of a larger F at every byte phase), destination layouts, every tile height -- the host's choices and each of 8, 4, 2, 1
    forced --, 0 / 255 noise, and the fuzz draws."""
    out = []
    rng = np.random.default_rng(29)

    def add(name, src, dst, cn, n=2, pad=0, off=0, gap=0, origin=None, margin=(0, 0), th=0, binary=False):
        (sw, sh), (dw, dh) = src, dst
        wx, wy = origin if origin is not None else (0, 0)
        C_, R_ = (sw + wx + margin[0], sh + wy + margin[1]) if origin is not None else (sw, sh)
        frames = rng.integers(0, 2, (n, R_, C_, cn), dtype=np.uint8) * 255 if binary else rng.integers(0, 256, (n, R_, C_, cn), dtype=np.uint8)
        out.append((FILTER_ID[name], R_, C_, wx, wy, sw, sh, dh, dw, cn, n, pad, off, gap, th, frames.astype(np.uint8)))
    for k, s in enumerate(AC.SHAPES):
        for name in NAMES:
            for cn in (1, 3):
                pad, off, gap = ((0, 0, 0), (5, 1, 3), (16, 3, 0))[(k + cn) % 3]
                add(name, s.src, s.dst, cn, pad=pad, off=off, gap=gap)
                origin = WINDOW_ORIGINS[(k + cn) % len(WINDOW_ORIGINS)]
                add(name, s.src, s.dst, cn, pad=pad, off=off, gap=gap, origin=origin, margin=((k % 3), (k % 2)))
    for origin in WINDOW_ORIGINS:                           # every phase under both channel counts, right up against F's last column
        for cn in (1, 3):
            add("cubic_aa", (50, 20), (21, 9), cn, origin=origin, margin=(0, 0))
            add("linear_aa", (50, 20), (70, 20), cn, origin=origin, margin=(1, 1))
    for name, cn, src, dst in AC.TILE_HEIGHT_SHAPES:
        add(name, src, dst, cn, n=1)
        add(name, src, dst, cn, n=1, origin=(1, 3), margin=(2, 1))
    for th in (8, 4, 2, 1):
        for cn in (1, 3):
            add("cubic_aa", (70, 90), (66, 19), cn, n=1, th=th)
            add("linear_aa", (8, 640), (8, 10), cn, n=1, th=th if cn == 1 or th <= 4 else 4)
    for cn in (1, 3):
        add("cubic_aa", (120, 90), (70, 41), cn, binary=True)
        add("cubic_aa", (40, 30), (90, 70), cn, binary=True)
    for seed in range(AC.FUZZ_CASES):
        k = AC.fuzz_case(seed)
        add(k["name"], k["src"], k["dst"], k["cn"], n=k["n"], pad=(0, 1, 16)[k["pitch"]], off=int(k["base_off"]), gap=5 if k["gap"] else 0,
            origin=(seed % 4, seed % 3) if seed % 2 else None, margin=(seed % 5, 1))
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_kernels_run_on_the_host_equal_the_reference_byte_for_byte(tmp_path, rip_lib, sanitize):
    """tests/cpp/aa_kernel_host.cpp: csrc/rip_aa.hip compiled as host code with the toolchain's clang++; per workgroup of the
    launcher's grid a heap block of exactly the launch's LDS size, phase 1 for all 256 threads, then phase 2; frames and tables in
    exactly sized heap blocks, destinations with sentinels.  The second build adds -fsanitize=address,undefined to this
    stand-alone program (no out-of-bounds access to a frame, a table or the LDS block, no misaligned wide access, no signed overflow)."""
    exe = build_host_program(tmp_path, "aa_kernel_host", ["aa_kernel_host.cpp", os.path.join(CSRC, "rip_output_tables.cpp")], stub="hip_host_stub_lds", sanitize=sanitize,
                             extra=["-ffp-contract=off", "-lm", "-lpthread"])
    cases = host_cases()
    assert len(cases) >= 150
    assert {c[14] for c in cases} >= {0, 1, 2, 4, 8} and {(c[3] * c[9]) % 4 for c in cases if c[9] == 3} == {0, 1, 2, 3}
    cases_path, out_path = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(cases_path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            f.write(struct.pack("<15i", *c[:15]))
            f.write(c[15].tobytes())
    r = subprocess.run([exe, cases_path, out_path], capture_output=True, text=True)
    assert r.returncode == 0 and "%d cases, 0 bad" % len(cases) in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.fromfile(out_path, np.uint8)
    name_of = {v: k for k, v in FILTER_ID.items()}
    at = 0
    for (flt, R_, C_, wx, wy, ww, wh, H, W, cn, n, pad, off, gap, th, frames) in cases:
        step = W * cn + pad
        frame = step * H + gap
        total = off + frame * (n - 1) + step * (H - 1) + W * cn
        want = np.full(total, 0xA5, np.uint8)
        for k in range(n):
            small = A.resize(frames[k, wy:wy + wh, wx:wx + ww], H, W, name_of[flt]).reshape(H, W * cn)
            for y in range(H):
                o = off + k * frame + y * step
                want[o:o + W * cn] = small[y]
        what = "%s %d x %d x %d window (%d, %d, %d, %d) -> %d x %d, %d frames, pad %d off %d gap %d th %d" % (name_of[flt], C_, R_, cn, wx, wy, ww, wh, W, H, n, pad, off, gap, th)
        assert np.array_equal(got[at:at + total], want), "%s: %d bytes differ" % (what, int((got[at:at + total] != want).sum()))
        at += total
    assert at == got.size
