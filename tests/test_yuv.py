"""The YUV 4:2:0 output formats "nv12" / "i420" (include/rip.h rip_set_output_yuv_matrix; PARITY.md "Output formats: YUV 4:2:0") without
a GPU: the definition's known answers and properties on tests/yuv_reference.py, an independent check against Pillow where it imports,
the setter / getter / YAML key per head, the queries on RIP_DEVICE_NONE handles against hand-computed values, the refusals and their
order, the C++ facade, and the kernel of csrc/rip_yuv.hip executed on the host thread by thread against the reference -- plainly, and
under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program.  Tolerance 0."""
import os
import struct
import subprocess

import numpy as np
import pytest

import output_reference
import yuv_reference as Y
from helpers import build_host_program
from raw_image_pipeline_amd import RawImagePipeline
from raw_image_pipeline_amd import pipeline as P
from test_cpp_facade import BRANCHES, run_env
from test_resize import write_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAYER = "bayer_rggb8"


def flat(b, g, r, h=2, w=2):
    return np.broadcast_to(np.array([b, g, r], np.uint8), (h, w, 3)).copy()


def one(b, g, r, matrix):
    y, cb, cr = Y.planes(flat(b, g, r), matrix)
    assert (y == y[0, 0]).all()
    return int(y[0, 0]), int(cb[0, 0]), int(cr[0, 0])


# ---- the definition -------------------------------------------------------------------------------------------------------------
KNOWN = {
    "bt601": ((81, 90, 240), (145, 54, 34), (41, 240, 110)),
    "bt709": ((63, 102, 240), (173, 42, 26), (32, 240, 118)),
    "bt601_full": ((76, 85, 255), (150, 44, 21), (29, 255, 107)),
}


@pytest.mark.parametrize("matrix", sorted(KNOWN))
def test_known_answers(matrix):
    red, green, blue = KNOWN[matrix]
    assert one(0, 0, 255, matrix) == red
    assert one(0, 255, 0, matrix) == green
    assert one(255, 0, 0, matrix) == blue


def test_a_block_of_red_green_blue_white_has_neutral_chroma():
    e = np.array([[[0, 0, 255], [0, 255, 0]], [[255, 0, 0], [255, 255, 255]]], np.uint8)
    y, cb, cr = Y.planes(e, "bt601")
    assert y.tolist() == [[81, 145], [41, 235]] and cb.tolist() == [[128]] and cr.tolist() == [[128]]


@pytest.mark.parametrize("matrix", Y.NAMES)
def test_grey_white_black(matrix):
    yoff, yw, cbw, crw = Y.MATRICES[matrix]
    full = matrix.endswith("_full")
    assert sum(yw) == (32768 if full else 28142) and sum(cbw) == 0 and sum(crw) == 0 and yoff == (0 if full else 16)
    for v in range(256):
        y, cb, cr = one(v, v, v, matrix)
        assert (cb, cr) == (128, 128)
        if full:
            assert y == v
    assert one(255, 255, 255, matrix)[0] == (255 if full else 235)
    assert one(0, 0, 0, matrix)[0] == (0 if full else 16)


@pytest.mark.parametrize("matrix", Y.NAMES)
def test_range_bounds(matrix):
    rng = np.random.default_rng(7)
    corners = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)], np.uint8)
    px = np.concatenate([corners, rng.integers(0, 256, (4096, 3), dtype=np.uint8)])
    e = np.repeat(np.repeat(px.reshape(-1, 1, 3), 2, axis=0), 2, axis=1).reshape(-1, 2, 3)      # every pixel as a flat 2 x 2 block
    y, cb, cr = Y.planes(e, matrix)
    if matrix.endswith("_full"):
        # the min binds for pure blue (Cb) and pure red (Cr) alone: 256 becomes 255
        assert one(255, 0, 0, matrix)[1] == 255 and one(0, 0, 255, matrix)[2] == 255
        yoff, yw, cbw, crw = Y.MATRICES[matrix]
        assert (cbw[0] * 1020 + (128 << 17) + 65536) >> 17 == 256 and (crw[2] * 1020 + (128 << 17) + 65536) >> 17 == 256
    else:
        assert y.min() >= 16 and y.max() <= 235 and cb.min() >= 16 and cb.max() <= 240 and cr.min() >= 16 and cr.max() <= 240
        assert {int(y.min()), int(y.max())} == {16, 235} and int(cb.max()) == 240 and int(cr.max()) == 240


def test_bt601_full_luma_is_mono8():
    e = np.random.default_rng(3).integers(0, 256, (64, 96, 3), dtype=np.uint8)
    assert np.array_equal(Y.planes(e, "bt601_full")[0], output_reference.mono8(e))


def test_layouts():
    e = np.random.default_rng(5).integers(0, 256, (6, 10, 3), dtype=np.uint8)
    y, cb, cr = Y.planes(e, "bt709")
    nv12, i420 = Y.convert(e, "nv12", "bt709"), Y.convert(e, "i420", "bt709")
    assert nv12.shape == i420.shape == (9, 10)
    assert np.array_equal(i420.reshape(-1), np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)]))      # contiguous I420
    assert np.array_equal(nv12[:6], y) and np.array_equal(nv12[6:, 0::2], cb) and np.array_equal(nv12[6:, 1::2], cr)
    for fmt, frame in (("nv12", nv12), ("i420", i420)):
        got = P.yuv_planes(frame, fmt)
        for a, b in zip(got, (y, cb, cr)):
            assert np.array_equal(a, b)
        assert np.array_equal(Y.pitched(e, fmt, "bt709", 10), frame.reshape(-1))
        batch = np.stack([frame, frame])
        assert all(np.array_equal(a[1], b) for a, b in zip(P.yuv_planes(batch, fmt), (y, cb, cr)))
    assert P.yuv_planes(nv12, "nv12")[1].strides[-1] == 2          # a strided view, no copy
    with pytest.raises(ValueError):
        P.yuv_planes(nv12, "nv21")
    with pytest.raises(ValueError):
        P.yuv_planes(nv12[:8], "nv12")


def test_against_pillow_where_it_imports():
    """An independent converter: Image.convert("YCbCr") is full-range BT.601 per pixel and truncates where this definition rounds, so
    on flat 2 x 2 blocks the planes agree within 1 level.  It rules out a wrong matrix, plane order or offset; it pins nothing."""
    try:
        from PIL import Image
    except ImportError:
        return
    rng = np.random.default_rng(11)
    px = rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)
    px[0, :8] = [[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)]
    e = np.repeat(np.repeat(px, 2, axis=0), 2, axis=1)
    y, cb, cr = Y.planes(e, "bt601_full")
    pil = np.asarray(Image.fromarray(np.ascontiguousarray(px[..., ::-1]), "RGB").convert("YCbCr")).astype(np.int64)
    assert np.abs(y[0::2, 0::2].astype(np.int64) - pil[..., 0]).max() <= 1
    assert np.abs(cb.astype(np.int64) - pil[..., 1]).max() <= 1
    assert np.abs(cr.astype(np.int64) - pil[..., 2]).max() <= 1


# ---- setter, getter, YAML ---------------------------------------------------------------------------------------------------------
def test_setter_getter_per_head(host_pipe):
    p = host_pipe
    assert p.get_output_yuv_matrix() == "bt601" and P.YUV_MATRICES == Y.NAMES
    assert P.YUV_OUTPUT_FORMATS == {"nv12": (np.uint8, False, 1), "i420": (np.uint8, False, 1)} and not set(P.YUV_OUTPUT_FORMATS) & set(P.OUTPUT_FORMATS)
    p.set_output_heads(3)
    for k, name in enumerate(("bt709", "bt601_full", "bt709_full")):
        p.select_output_head(k)
        p.set_output_yuv_matrix(name)
    for k, name in enumerate(("bt709", "bt601_full", "bt709_full")):
        p.select_output_head(k)
        assert p.get_output_yuv_matrix() == name
    for bad in ("bt2020", "BT601", "", "bt601 ", "full"):
        with pytest.raises(ValueError, match="'bt601', 'bt709', 'bt601_full', 'bt709_full'"):
            p.set_output_yuv_matrix(bad)
        assert p.get_output_yuv_matrix() == "bt709_full"
    assert p._lib.rip_set_output_yuv_matrix(p._h, None) == P.RIP_ERR_INVALID_ARGUMENT
    assert p._lib.rip_set_output_yuv_matrix(None, b"bt601") == P.RIP_ERR_INVALID_ARGUMENT
    # rip_set_output_heads resets it for the heads it resets
    p.set_output_heads(1)
    p.set_output_heads(3)
    for k, name in enumerate(("bt709", "bt601", "bt601")):
        p.select_output_head(k)
        assert p.get_output_yuv_matrix() == name
    # the unknown-format message keeps its shape and lists the new names behind the old ones
    with pytest.raises(ValueError, match="Supported formats: 'native', 'rgb8', .*'bgr_chw_bf16', 'nv12', 'i420'"):
        p.set_output_format("nv21")


def test_yaml_key(tmp_path, host_pipe):
    p = host_pipe
    p.load_params(write_params(tmp_path, "output:\n  format: nv12\n  yuv_matrix: bt709\noutput_1:\n  format: i420\n  yuv_matrix: bt601_full\noutput_2:\n  format: rgb8\n"))
    assert p.get_output_heads() == 3
    for k, (fmt, name) in enumerate((("nv12", "bt709"), ("i420", "bt601_full"), ("rgb8", "bt601"))):
        p.select_output_head(k)
        assert (p.get_output_format(), p.get_output_yuv_matrix()) == (fmt, name)
    p.load_params(write_params(tmp_path, "output:\n  format: nv12\n"))          # absent: bt601
    assert p.get_output_yuv_matrix() == "bt601" and p.get_output_format() == "nv12"


@pytest.mark.parametrize("text", ["output:\n  yuv_matrix: bt2020\n", "output:\n  yuv_matrix: [1, 2]\n", "output:\n  format: nv12\noutput_1:\n  yuv_matrix: 601\n"])
def test_yaml_invalid_value_fails_and_changes_nothing(tmp_path, host_pipe, text):
    p = host_pipe
    p.set_output_yuv_matrix("bt709_full")
    p.set_flip(True)
    with pytest.raises(ValueError):
        p.load_params(write_params(tmp_path, "flip:\n  enabled: false\n" + text))
    assert p.get_output_yuv_matrix() == "bt709_full" and p.is_flip_enabled() and p.get_output_format() == "native"


@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade(tmp_path, rip_lib, branch):
    exe = str(tmp_path / ("yuv_test_" + branch.replace("-", "_")))
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror"] + BRANCHES[branch] + ["-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "yuv_test.cpp"), "-o", exe, "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir,
           "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "host"], capture_output=True, text=True, env=run_env(-1))
    assert r.returncode == 0 and "yuv host OK" in r.stdout, r.stdout + r.stderr


# ---- the queries on a handle without a device ---------------------------------------------------------------------------------------
# (settings, picture (W, H), window read, rectangle written) for a 136 x 72 Bayer frame, by hand: no target: F itself; a stretch to
# 64 x 48; a letterbox of 136 x 72 into 64 x 48: scale min(64/136, 48/72) = 0.4706 -> 64 x 34, centred: top (48 - 34) / 2 = 7; a
# window of 64 x 32 at (8, 4) without a target
GEOMETRIES = [
    (dict(), (136, 72), (0, 0, 136, 72), (0, 0, 136, 72)),
    (dict(size=(64, 48)), (64, 48), (0, 0, 136, 72), (0, 0, 64, 48)),
    (dict(size=(64, 48), fit="letterbox"), (64, 48), (0, 0, 136, 72), (0, 7, 64, 34)),
    (dict(roi=(8, 4, 64, 32)), (64, 32), (8, 4, 64, 32), (0, 0, 64, 32)),
]


def configure_geometry(p, g):
    p.set_output_size(*g.get("size", (0, 0)))
    p.set_output_fit(g.get("fit", "stretch"))
    p.set_output_roi(*g.get("roi", (0, 0, 0, 0)))


@pytest.mark.parametrize("fmt", Y.FORMATS)
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=["plain", "target", "letterbox", "window"])
def test_queries_under_every_selection(rip_lib, fmt, geometry):
    settings, (w, h), src, dst = geometry
    p = RawImagePipeline(False, "", "", "", device=-1)
    p.set_undistortion(False)
    p.set_output_heads(3)
    twin = RawImagePipeline(False, "", "", "", device=-1)      # the same geometry under "native": what describes the picture
    twin.set_undistortion(False)
    configure_geometry(twin, settings)
    for k in range(3):
        p.select_output_head(k)
        configure_geometry(p, settings if k == 1 else {})
        p.set_output_format(fmt if k == 1 else "native")
    for k in range(3):
        p.select_output_head(k)
        if k != 1:
            assert p.query_output(72, 136, 1, BAYER) == (72, 136, 3, "bgr8")
            assert p.query_output_bytes(72, 136, 1, BAYER) == (72 * 136 * 3, 1, 0)
            continue
        assert p.query_output(72, 136, 1, BAYER) == (3 * h // 2, w, 1, fmt)
        assert p.query_output_bytes(72, 136, 1, BAYER) == (3 * h * w // 2, 1, 0)
        assert p.get_output_window(72, 136, 1, BAYER) == (src, dst) == twin.get_output_window(72, 136, 1, BAYER)
        ih, iw, K, Pm = p.get_output_camera_info(72, 136, 1, BAYER)
        th, tw, tK, tP = twin.get_output_camera_info(72, 136, 1, BAYER)
        assert (ih, iw) == (h, w) == (th, tw) and np.array_equal(K, tK) and np.array_equal(Pm, tP)
        p.set_rect_mask("coverage")
        st_h, st_w = P.C.c_int(), P.C.c_int()
        assert p._lib.rip_get_output_mask(p._h, 72, 136, 1, BAYER.encode(), None, P.C.c_size_t(0), P.C.byref(st_h), P.C.byref(st_w)) == P.RIP_OK
        assert (st_h.value, st_w.value) == (h, w)


# ---- the refusals and their order --------------------------------------------------------------------------------------------------
def all_queries(p, rows, cols, channels, enc):
    return [lambda: p.query_output(rows, cols, channels, enc), lambda: p.query_output_bytes(rows, cols, channels, enc),
            lambda: p.get_output_camera_info(rows, cols, channels, enc), lambda: p.get_output_window(rows, cols, channels, enc)]


@pytest.mark.parametrize("fmt", Y.FORMATS)
def test_refusals_and_their_order(host_pipe, fmt):
    p = host_pipe
    for off in (p.set_undistortion, p.set_white_balance, p.set_vignetting_correction, p.set_color_calibration, p.set_gamma_correction,
                p.set_color_enhancer, p.set_flip):
        off(False)
    p.set_output_format(fmt)
    # 1. the existing format rules first: a bgr16 result, then a one-channel result -- on frames that are odd-sized too
    p.set_debayer_16bit(True)
    for q in all_queries(p, 71, 135, 1, "bayer_rggb16"):
        with pytest.raises(ValueError, match="needs an 8-bit pipeline result"):
            q()
    for q in all_queries(p, 33, 65, 1, "mono8"):
        with pytest.raises(ValueError, match="needs a three-channel pipeline result"):
            q()
    # 2. an odd width or height of the delivered picture, named
    for rows, cols in ((71, 136), (72, 135), (71, 135)):
        for q in all_queries(p, rows, cols, 1, BAYER):
            with pytest.raises(ValueError, match="even width and height.*%d x %d" % (cols, rows)):
                q()
    # ... of the DELIVERED picture: an odd frame behind an even target passes, an even frame behind an odd target or window does not
    p.set_output_size(64, 48)
    assert p.query_output(71, 135, 1, BAYER) == (72, 64, 1, fmt)
    p.set_output_size(63, 48)
    with pytest.raises(ValueError, match="63 x 48"):
        p.query_output(72, 136, 1, BAYER)
    p.set_output_size(0, 0)
    p.set_output_roi(8, 4, 64, 31)
    with pytest.raises(ValueError, match="64 x 31"):
        p.query_output(72, 136, 1, BAYER)
    # the heads calls' checks run per head under its own selection: the Python binding names the head as the C ABI does
    p.set_output_roi(0, 0, 0, 0)
    p.set_output_heads(2)
    p.select_output_head(1)
    p.set_output_format(fmt)
    p.select_output_head(0)
    p.set_output_format("native")
    with pytest.raises(ValueError, match="output head 1: .*even width and height"):
        p._head_queries([0, 1], 71, 136, 1, BAYER)
    # no effect under any other format
    p.set_output_yuv_matrix("bt709")
    assert p.query_output(71, 135, 1, BAYER) == (71, 135, 3, "bgr8")


# ---- the kernel on the host --------------------------------------------------------------------------------------------------------
HOST_WIDTHS = (2, 4, 6, 8, 10, 14, 16, 18, 510, 514)      # 512 columns are a workgroup's span (rip_yuv.hpp kYuvPxPerBlockX)
HOST_HEIGHTS = (2, 4, 6, 66)


def host_cases():
    """(rows, cols, semi, src_pitch, dst_pitch, dst_off, frames, matrix name, seed): every width x height of the GPU test with both
    formats at a tight pitch; then pitches (tight, 4-aligned source with a 16-byte destination, odd / even-not-4) x bases 0..3."""
    cases = []
    seed = 0
    for w in HOST_WIDTHS:
        for h in HOST_HEIGHTS:
            for semi in (1, 0):
                seed += 1
                cases.append((h, w, semi, (3 * w + 3) & ~3, w, 0, 1, Y.NAMES[seed % 4], seed))
    for w, h in ((18, 6), (14, 4), (16, 10), (514, 6)):
        for semi in (1, 0):
            for src_pitch, dst_pitch in (((3 * w + 3) & ~3, w), ((3 * w + 15) & ~15, (w + 15) & ~15), ((3 * w + 3 & ~3) + 4, w + (3 if semi else 2))):
                for off in range(4):
                    seed += 1
                    cases.append((h, w, semi, src_pitch, dst_pitch, off, 3 if off == 2 else 1, Y.NAMES[seed % 4], seed))
    return cases


def frame_total(h, w, semi, pitch):
    """bytes from the frame's start to behind the last byte its layout holds"""
    if semi:
        return (3 * h // 2 - 1) * pitch + w
    return h * pitch + (h // 2) * (pitch // 2) + (h // 2 - 1) * (pitch // 2) + w // 2


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_kernel_run_on_the_host_equals_the_reference(tmp_path, sanitize):
    """tests/cpp/yuv_kernel_host.cpp: csrc/rip_yuv.hip compiled as host code with the toolchain's clang++, every thread of the
    launcher's grid run in turn from exactly sized sources into exactly sized destinations with sentinels around every row.
    The second build adds -fsanitize=address,undefined to this stand-alone program."""
    exe = build_host_program(tmp_path, "yuv_kernel_host", ["yuv_kernel_host.cpp"], sanitize=sanitize, extra=["-Wall"])
    cases = host_cases()
    assert len(cases) == 10 * 4 * 2 + 4 * 2 * 3 * 4
    cases_path, out_path = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    wants = []
    with open(cases_path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for (h, w, semi, sp, dp, off, frames, name, seed) in cases:
            rng = np.random.default_rng(seed)
            stride = dp * (3 * h // 2) + 5
            total = stride * (frames - 1) + frame_total(h, w, semi, dp)
            yoff, yw, cbw, crw = Y.MATRICES[name]
            f.write(struct.pack("<8i", h, w, semi, sp, dp, off, total, frames))
            f.write(struct.pack("<10i", *(yw + cbw + crw + (yoff,))))
            src = rng.integers(0, 256, (frames, h, sp), dtype=np.uint8)      # the pitch bytes are random too: nothing of them may show
            if seed % 5 == 0:
                src[:, :, :3 * w] = np.array([255, 0, 0] if seed % 2 else [0, 0, 255], np.uint8).tolist() * w      # where the full-range min binds
            f.write(src.reshape(-1)[:sp * h * (frames - 1) + sp * (h - 1) + ((3 * w + 3) & ~3)].tobytes())
            want = np.full(off + total, 0xA5, np.uint8)
            for k in range(frames):
                e = src[k, :, :3 * w].reshape(h, w, 3)
                one_frame = Y.pitched(e, "nv12" if semi else "i420", name, dp, total=frame_total(h, w, semi, dp), base=0)
                at = off + k * stride
                written = one_frame != 0xA5
                # the layout's own bytes, sentinel-valued results included: lay the frame over the block through a mask of its positions
                mask = Y.pitched(np.zeros_like(e), "nv12" if semi else "i420", "bt601_full", dp, fill=1, total=frame_total(h, w, semi, dp)) != 1
                assert (written <= mask).all()
                want[at:at + one_frame.size][mask] = one_frame[mask]
            wants.append(want)
    r = subprocess.run([exe, cases_path, out_path], capture_output=True, text=True)
    assert r.returncode == 0 and "%d cases, 0 bad" % len(cases) in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.fromfile(out_path, np.uint8)
    at = 0
    for c, want in zip(cases, wants):
        assert np.array_equal(got[at:at + want.size], want), "%r: %d bytes differ" % (c[:8], int((got[at:at + want.size] != want).sum()))
        at += want.size
    assert at == got.size
