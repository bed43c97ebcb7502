"""The output format "jpeg" (include/rip.h rip_set_output_jpeg; PARITY.md "Output formats: JPEG") without a GPU: the reference's reader
against its writer, the forward DCT's condition, the reciprocal tables against the division, an independent pin against Pillow where
it imports, the setter / getter / YAML keys per head, the queries and the slot formula on RIP_DEVICE_NONE handles, the refusals and
their order, the C++ facade, and the four kernels of csrc/rip_jpeg.hip executed on the host thread by thread against the reference --
plainly, and as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer.  Tolerance 0."""
import io
import os
import struct
import subprocess
import warnings

import numpy as np
import pytest

from helpers import build_host_program
import jpeg_reference as JR
from raw_image_pipeline_amd import pipeline as P
from test_cpp_facade import BRANCHES, run_env
from test_resize import write_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAYER = "bayer_rggb8"
# measured here (test_pillow_decodes_what_the_reference_reconstructs prints it): Pillow's integer IDCT against the float64 one
PILLOW_MAX_DIFF = 1


def pictures():
    rng = np.random.default_rng(1)
    out = []
    for shape in ((8, 8), (17, 9), (9, 17, 3), (1, 1, 3), (1, 1), (40, 56, 3), (33, 70), (16, 208, 3)):
        out.append(rng.integers(0, 256, shape, dtype=np.uint8))
    g = ((np.arange(50)[None, :] * 5 + np.arange(30)[:, None] * 3) % 256).astype(np.uint8)
    out += [g, np.stack([g, 255 - g, g // 2], -1), np.full((20, 20, 3), (10, 200, 90), np.uint8), ((np.indices((24, 24)).sum(0) % 2) * 255).astype(np.uint8)]
    return out


# ---- the definition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality,restart_rows", [(1, 1), (50, 2), (90, 1), (100, 64)])
def test_the_reader_returns_what_the_writer_coded(quality, restart_rows):
    for pic in pictures():
        s = JR.encode(pic, quality, restart_rows)
        dec = JR.decode_coefficients(s)
        ncomp = 1 if pic.ndim == 2 else 3
        assert dec["length"] == len(s) and (dec["height"], dec["width"]) == pic.shape[:2]
        assert dec["markers"] == [0xD8, 0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA] and s[:JR.HEADER_BYTES[ncomp]] == JR.header(*pic.shape[:2], ncomp, quality, restart_rows)
        mcu = 8 if ncomp == 1 else 16
        assert dec["restart_interval"] == restart_rows * -(-pic.shape[1] // mcu)
        assert len(dec["restarts"]) == -(-(-(-pic.shape[0] // mcu)) // restart_rows) - 1
        for got, want in zip(dec["blocks"], JR.component_blocks(pic, quality)):
            assert np.array_equal(got, want)
        assert all(np.abs(b[:, 1:]).max(initial=0) <= 1023 and np.abs(np.diff(b[:, 0], prepend=0)).max() <= 2047 for b in dec["blocks"])
        assert len(s) <= JR.default_slot(*pic.shape[:2], ncomp, restart_rows) or quality == 100


def test_the_planes_are_the_yuv_references_of_the_extended_picture():
    import yuv_reference as Y
    pic = np.random.default_rng(3).integers(0, 256, (9, 17, 3), dtype=np.uint8)
    ext = JR.extend(pic, 16)
    assert ext.shape == (16, 32, 3) and (ext[:9, :17] == pic).all() and (ext[9:, :17] == pic[8:9]).all() and (ext[:, 17:] == ext[:, 16:17]).all()
    for got, want in zip(JR.planes(pic), Y.planes(ext, "bt601_full")):
        assert np.array_equal(got, want)
    grey = pic[..., 1].copy()
    assert np.array_equal(JR.planes(grey)[0], JR.extend(grey, 8))


def dct_blocks():
    rng = np.random.default_rng(2)
    checker = (np.indices((8, 8)).sum(0) % 2) * 255
    impulses = np.zeros((128, 8, 8), np.int64)
    for i in range(64):
        impulses[i].flat[i] = 255
        impulses[64 + i] = 255
        impulses[64 + i].flat[i] = 0
    return np.concatenate([rng.integers(0, 256, (2000, 8, 8)), np.full((1, 8, 8), 0), np.full((1, 8, 8), 255), np.full((1, 8, 8), 77), checker[None], 255 - checker[None], impulses])


def test_the_forward_dct_stays_within_one_of_the_float_dct():
    """PARITY.md: on random, flat, 0 / 255 checkerboard and single-impulse blocks the unquantised coefficients stay within 1.0 of
    scipy's orthonormal DCT-II of block - 128.  Measured: 0.155."""
    from scipy.fft import dctn
    b = dct_blocks()
    c8 = JR.fdct(b)
    err = np.abs(c8 / 8.0 - dctn(b - 128.0, axes=(1, 2), norm="ortho")).max()
    print("forward DCT: max |coefficient - float| = %.4f" % err)
    assert err <= 1.0
    assert np.abs(c8).max() <= 8192          # |c| + 4 Q stays below 2^16, the range the reciprocals are exact on


@pytest.mark.parametrize("quality", [1, 10, 50, 75, 90, 95, 100])
def test_the_reciprocal_tables_equal_the_division(rip_lib, quality):
    q, recip, half = np.zeros(128, np.uint8), np.zeros(128, np.uint32), np.zeros(128, np.uint32)
    st = rip_lib.rip_debug_jpeg_tables(int(quality), q.ctypes.data_as(P.C.c_void_p), recip.ctypes.data_as(P.C.c_void_p), half.ctypes.data_as(P.C.c_void_p))
    assert st == P.RIP_OK
    ql, qc = JR.quant_tables(quality)
    assert np.array_equal(q[:64], ql) and np.array_equal(q[64:], qc) and np.array_equal(half, 4 * q.astype(np.uint32))
    assert [int(r) for r in recip] == [JR.reciprocal(v) for v in q]
    a = np.arange(1 << 16, dtype=np.uint64)          # every value |c| + 4 Q can take, and beyond
    for v in sorted(set(int(x) for x in q)):
        assert np.array_equal((a * np.uint64(JR.reciprocal(v))) >> np.uint64(32), a // np.uint64(8 * v)), v


def test_every_divisor_has_an_exact_reciprocal():
    a = np.arange(1 << 16, dtype=np.uint64)
    for v in range(1, 256):
        assert np.array_equal((a * np.uint64(JR.reciprocal(v))) >> np.uint64(32), a // np.uint64(8 * v)), v


def test_quantisation_rounds_ties_away_from_zero():
    q = np.full(64, 3)
    c = np.zeros((8, 8), np.int64)
    c.flat[:8] = [12, -12, 11, -11, 36, -36, 35, -35]          # 8 Q = 24: 0.5, 0.458, 1.5, 1.458
    assert JR.quantise(c, q).flat[:8].tolist() == [1, -1, 0, 0, 2, -2, 1, -1]
    c.flat[0] = -8192
    assert JR.quantise(c, np.ones(64)).flat[0] == -1023          # the clamp


# ---- an independent binary -----------------------------------------------------------------------------------------------------------
def pillow_segments(data):
    """{(class, id): (bits, vals)} and {id: divisors in natural order} of a file Pillow wrote."""
    pos, huff, quant = 2, {}, {}
    while True:
        m, n = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        seg = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        if m == 0xC4:
            while seg:
                bits = list(seg[1:17])
                huff[(seg[0] >> 4, seg[0] & 15)] = (bits, list(seg[17:17 + sum(bits)]))
                seg = seg[17 + sum(bits):]
        elif m == 0xDB:
            while seg:
                t = np.zeros(64, np.int64)
                t[JR.ZIGZAG] = list(seg[1:65])
                quant[seg[0] & 15] = t
                seg = seg[65:]
        elif m == 0xDA:
            return huff, quant


def test_the_tables_are_the_ones_pillow_writes():
    Image = pytest.importorskip("PIL.Image")
    pic = np.random.default_rng(4).integers(0, 256, (32, 32, 3), dtype=np.uint8)
    for quality in (1, 10, 50, 75, 90, 95, 100):
        buf = io.BytesIO()
        Image.fromarray(pic).save(buf, "JPEG", quality=quality, optimize=False)
        huff, quant = pillow_segments(buf.getvalue())
        assert huff == {(0, 0): JR.DC_LUMA, (0, 1): JR.DC_CHROMA, (1, 0): JR.AC_LUMA, (1, 1): JR.AC_CHROMA}
        ql, qc = JR.quant_tables(quality)
        assert np.array_equal(quant[0], ql) and np.array_equal(quant[1], qc)
        ours = Image.open(io.BytesIO(JR.encode(pic, quality, 1)))
        theirs = Image.open(io.BytesIO(buf.getvalue()))
        assert ours.quantization == theirs.quantization
    assert np.array_equal(JR.quant_tables(50)[0], JR.BASE_LUMA) and np.array_equal(JR.quant_tables(50)[1], JR.BASE_CHROMA)


def test_pillow_decodes_what_the_reference_reconstructs():
    """Pillow opens every reference stream without a warning and reports the true size and mode; its decoded grey pixels, and the Y
    plane of its draft('YCbCr') decode of a colour stream, differ from the reference's own float64 reconstruction by the decoder's
    integer IDCT alone.  Chroma is compared on pictures whose chroma is flat (no upsampling filter to agree on)."""
    Image = pytest.importorskip("PIL.Image")
    worst = 0
    for quality, restart_rows in ((1, 1), (50, 2), (90, 1), (100, 64)):
        for pic in pictures():
            s = JR.encode(pic, quality, restart_rows)
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                im = Image.open(io.BytesIO(s))
                im.load()
            h, w = pic.shape[:2]
            assert im.size == (w, h) and im.mode == ("L" if pic.ndim == 2 else "RGB")
            rec = JR.reconstruct(JR.decode_coefficients(s))
            im = Image.open(io.BytesIO(s))
            if pic.ndim == 3:
                im.draft("YCbCr", im.size)
                assert im.mode == "YCbCr"
            px = np.asarray(im).astype(np.int64)
            y = px if px.ndim == 2 else px[..., 0]
            worst = max(worst, int(np.abs(y - rec[0][:h, :w]).max()))
            if pic.ndim == 3 and (pic == pic[0, 0]).all():          # flat chroma
                for c in (1, 2):
                    assert (rec[c] == rec[c][0, 0]).all()
                    worst = max(worst, int(np.abs(px[..., c] - int(rec[c][0, 0])).max()))
    print("Pillow against the float64 reconstruction: max difference %d" % worst)
    assert worst <= PILLOW_MAX_DIFF + 1


# ---- settings ----------------------------------------------------------------------------------------------------------------------
def test_setter_getter_per_head(host_pipe):
    p = host_pipe
    assert p.get_output_jpeg() == (90, 1)
    assert P.JPEG_OUTPUT_FORMATS == {"jpeg": (np.uint8, False, 1)} and "jpeg" not in P.OUTPUT_FORMATS and "jpeg" not in P.YUV_OUTPUT_FORMATS
    p.set_output_heads(3)
    values = ((1, 64), (100, 1), (55, 7))
    for k, v in enumerate(values):
        p.select_output_head(k)
        p.set_output_jpeg(*v)
    for k, v in enumerate(values):
        p.select_output_head(k)
        assert p.get_output_jpeg() == v
    for bad in ((0, 1), (101, 1), (-1, 1), (90, 0), (90, 65), (90, -3)):
        with pytest.raises(ValueError, match="output jpeg"):
            p.set_output_jpeg(*bad)
        assert p.get_output_jpeg() == (55, 7)
    assert p._lib.rip_set_output_jpeg(None, 90, 1) == P.RIP_ERR_INVALID_ARGUMENT
    assert p._lib.rip_get_output_jpeg(p._h, None, None) == P.RIP_OK
    p.set_output_heads(1)                  # rip_set_output_heads resets it for the heads it resets
    p.set_output_heads(3)
    assert [p.select_output_head(k) or p.get_output_jpeg() for k in range(3)] == [(1, 64), (90, 1), (90, 1)]
    with pytest.raises(ValueError, match="Supported formats: .*'i420', 'jpeg'"):
        p.set_output_format("jpg")
    with pytest.raises(P.RipError):          # the lengths live on the device
        p.jpeg_sizes()


def test_yaml_keys(tmp_path, host_pipe):
    p = host_pipe
    p.load_params(write_params(tmp_path, "output:\n  format: jpeg\n  jpeg_quality: 75\n  jpeg_restart_rows: 4\noutput_1:\n  format: rgb8\noutput_2:\n  jpeg_quality: 100\n"))
    assert p.get_output_heads() == 3 and p.get_output_format() == "jpeg"
    for k, v in enumerate(((75, 4), (90, 1), (100, 1))):
        p.select_output_head(k)
        assert p.get_output_jpeg() == v
    p.load_params(write_params(tmp_path, "output:\n  format: jpeg\n"))          # absent: the defaults
    assert p.get_output_jpeg() == (90, 1) and p.get_output_format() == "jpeg"


@pytest.mark.parametrize("text", ["output:\n  jpeg_quality: 0\n", "output:\n  jpeg_quality: 101\n", "output:\n  jpeg_quality: 90.5\n", "output:\n  jpeg_restart_rows: 65\n",
                                  "output:\n  jpeg_restart_rows: 0\n", "output:\n  format: jpeg\noutput_1:\n  jpeg_restart_rows: -1\n"])
def test_yaml_invalid_value_fails_and_changes_nothing(tmp_path, host_pipe, text):
    p = host_pipe
    p.set_output_jpeg(33, 3)
    p.set_flip(True)
    with pytest.raises(ValueError, match="jpeg"):
        p.load_params(write_params(tmp_path, "flip:\n  enabled: false\n" + text))
    assert p.get_output_jpeg() == (33, 3) and p.is_flip_enabled() and p.get_output_heads() == 1


# ---- queries and refusals on a handle without a device ----------------------------------------------------------------------------
def off(p):
    for s in (p.set_undistortion, p.set_white_balance, p.set_vignetting_correction, p.set_color_calibration, p.set_gamma_correction, p.set_color_enhancer, p.set_flip):
        s(False)


@pytest.mark.parametrize("size,channels,restart_rows,slot", [
    ((8, 8), 1, 1, 330 + 64 + 2 + 2), ((16, 16), 3, 1, 613 + 384 + 2 + 2), ((17, 9), 3, 1, 613 + 32 * 16 * 3 // 2 + 2 + 2), ((9, 17), 1, 2, 330 + 16 * 24 + 2 * 2 + 2),
    ((1, 1), 3, 64, 613 + 384 + 2 + 2), ((2448, 2048), 3, 1, 613 + 2448 * 2048 * 3 // 2 + 2 * 128 + 2), ((2448, 2048), 1, 5, 330 + 2448 * 2048 + 2 * 52 + 2)])
def test_the_queries_report_one_slot(host_pipe, size, channels, restart_rows, slot):
    p = host_pipe
    off(p)
    w, h = size
    enc = "mono8" if channels == 1 else "bgr8"
    p.set_output_format("jpeg")
    p.set_output_jpeg(90, restart_rows)
    assert JR.default_slot(h, w, channels, restart_rows) == slot
    assert p.query_output(h, w, channels, enc) == (1, slot, 1, "jpeg") and p.query_output_bytes(h, w, channels, enc) == (slot, 1, False)
    p.set_output_jpeg(1, restart_rows)          # the quality does not change the slot
    assert p.query_output(h, w, channels, enc) == (1, slot, 1, "jpeg")
    p.set_output_yuv_matrix("bt709")            # without effect
    assert p.query_output(h, w, channels, enc) == (1, slot, 1, "jpeg")


def test_the_picture_keeps_its_description(host_pipe):
    """rip_get_output_window and rip_get_output_camera_info describe the picture, whatever the format delivers it in; a Bayer frame is
    a three-component stream behind a resize, a window and a letterbox."""
    p = host_pipe
    off(p)
    for settings, pic in ((dict(), (136, 72)), (dict(size=(63, 47)), (63, 47)), (dict(roi=(8, 4, 61, 31)), (61, 31)), (dict(size=(64, 48), fit="letterbox"), (64, 48))):
        p.set_output_size(*settings.get("size", (0, 0)))
        p.set_output_roi(*settings.get("roi", (0, 0, 0, 0)))
        p.set_output_fit(settings.get("fit", "stretch"))
        p.set_output_format("native")
        window = p.get_output_window(72, 136, 1, BAYER)
        assert p.query_output(72, 136, 1, BAYER)[:3] == (pic[1], pic[0], 3)
        p.set_output_format("jpeg")
        assert p.get_output_window(72, 136, 1, BAYER) == window
        assert p.query_output(72, 136, 1, BAYER) == (1, JR.default_slot(pic[1], pic[0], 3, 1), 1, "jpeg")


def test_refusals_and_their_order(host_pipe):
    p = host_pipe
    off(p)
    p.set_output_format("jpeg")
    p.set_debayer_16bit(True)
    p.set_output_clahe(2.0, 4, 4)
    p.set_output_roi(200, 0, 16, 16)
    with pytest.raises(ValueError, match="output roi / fit need an 8-bit pipeline result"):          # the resize's refusals come first
        p.query_output(72, 136, 1, "bayer_rggb16")
    p.set_output_roi(0, 0, 0, 0)
    with pytest.raises(ValueError, match=r"output format \[jpeg\] needs an 8-bit pipeline result"):          # bgr16, in the words of every format
        p.query_output(72, 136, 1, "bayer_rggb16")
    p.set_output_roi(200, 0, 16, 16)
    with pytest.raises(ValueError, match="roi"):          # a window outside F, before CLAHE
        p.query_output(72, 136, 1, BAYER)
    p.set_output_roi(0, 0, 0, 0)
    for enc, cn in ((BAYER, 1), ("mono8", 1)):
        with pytest.raises(ValueError, match=r"output format \[jpeg\] does not take CLAHE"):
            p.query_output(72, 136, cn, enc)
        with pytest.raises(ValueError, match="does not take CLAHE"):
            p.query_output_bytes(72, 136, cn, enc)
    p.set_output_clahe(0.0, 0, 0)
    assert p.query_output(72, 136, 1, "mono8")[3] == "jpeg"
    p.set_output_jpeg(90, 64)          # 64 rows of 1025 MCUs: beyond DRI's 16 bits
    with pytest.raises(ValueError, match="65535 MCUs a restart interval holds"):
        p.query_output(16, 16400, 3, "bgr8")
    p.set_output_jpeg(90, 1)
    with pytest.raises(ValueError, match="65535 pixels per side"):
        p.query_output(65536, 8, 1, "mono8")
    p.set_output_heads(2)
    p.select_output_head(1)
    p.set_output_format("jpeg")
    p.set_output_clahe(2.0, 4, 4)
    with pytest.raises(ValueError, match="does not take CLAHE"):
        p.query_output(72, 136, 1, BAYER)
    p.select_output_head(0)
    assert p.query_output(72, 136, 1, BAYER)[3] == "jpeg"


def test_jpeg_streams_cuts_slots():
    slots = np.arange(30, dtype=np.uint8).reshape(3, 10)
    assert P.jpeg_streams(slots, [4, 0, 10]) == [bytes([0, 1, 2, 3]), b"", bytes(range(20, 30))]
    with pytest.raises(ValueError):
        P.jpeg_streams(slots, [1, 2])


# ---- the facade --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade(tmp_path, rip_lib, branch):
    exe = str(tmp_path / ("jpeg_test_" + branch.replace("-", "_")))
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror"] + BRANCHES[branch] + ["-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "jpeg_test.cpp"), "-o", exe, "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir,
           "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "host"], capture_output=True, text=True, env=run_env(-1))
    assert r.returncode == 0 and "jpeg host OK" in r.stdout, r.stdout + r.stderr


# ---- the kernels on the host ---------------------------------------------------------------------------------------------------------
def host_cases():
    """dicts: shape, quality, restart rows, frames' pictures, slot, frame stride, base offset of the destination, source pitch"""
    rng = np.random.default_rng(5)
    cases = []

    def add(shape, q, rr, frames=1, slot=None, gap=0, off=0, pitch_extra=0, kind="noise"):
        h, w = shape[:2]
        ch = 1 if len(shape) == 2 else 3
        pics = []
        for _ in range(frames):
            if kind == "noise":
                pic = rng.integers(0, 256, shape, dtype=np.uint8)
            elif kind == "flat":
                pic = np.full(shape, int(rng.integers(0, 256)), np.uint8)
            else:
                pic = ((np.indices((h, w)).sum(0) % 2) * 255).astype(np.uint8)
                pic = pic if ch == 1 else np.repeat(pic[..., None], 3, 2)
            pics.append(np.ascontiguousarray(pic))
        slot = slot or JR.default_slot(h, w, ch, rr)
        cases.append(dict(shape=shape, ch=ch, q=q, rr=rr, pics=pics, slot=slot, stride=slot + gap, off=off, pitch=w * ch + pitch_extra))

    add((8, 8), 90, 1)
    add((16, 16, 3), 90, 1)
    add((17, 9, 3), 50, 1, frames=2, off=3, gap=5)
    add((9, 17), 90, 2, off=1, pitch_extra=3)
    add((1, 1, 3), 90, 1)
    add((1, 1), 1, 64)
    add((16, 208, 3), 90, 1)
    add((8, 520), 90, 1)
    add((144, 8), 90, 1, off=7)
    add((40, 56, 3), 100, 2, kind="checker")
    add((40, 56), 1, 1, kind="checker")
    add((24, 24, 3), 90, 64, kind="flat")
    add((32, 32, 3), 100, 1, frames=3)          # overflow in the middle of flat neighbours
    cases[-1]["pics"][0][:] = 9
    cases[-1]["pics"][2][:] = 99
    add((32, 32, 3), 100, 1, slot=8000)
    add((2100, 24), 90, 1, kind="flat")          # more intervals than one workgroup of the sizing and writing passes has
    return cases


def run_host_kernels(tmp_path, sanitize):
    exe = build_host_program(tmp_path, "jpeg_kernel_host", ["jpeg_kernel_host.cpp"], sanitize=sanitize, extra=["-Wall"])
    cases = host_cases()
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            h, w = c["shape"][:2]
            f.write(struct.pack("<10i", h, w, c["ch"], c["q"], c["rr"], len(c["pics"]), c["slot"], c["stride"], c["off"], c["pitch"]))
            for pic in c["pics"]:
                buf = np.full((h, c["pitch"]), 0x5A, np.uint8)
                buf[:, :w * c["ch"]] = pic.reshape(h, -1)
                f.write(buf.tobytes())
    r = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and "%d cases, 0 bad" % len(cases) in r.stdout, r.stdout + r.stderr
    out, pos, overflowed = np.fromfile(tmp_path / "out.bin", np.uint8), 0, 0
    for i, c in enumerate(cases):
        n = len(c["pics"])
        sizes = out[pos:pos + 4 * n].view(np.uint32)
        pos += 4 * n
        total = c["off"] + c["stride"] * (n - 1) + c["slot"] + 7
        got = out[pos:pos + total]
        pos += total
        want, want_sizes = np.full(total, 0xA5, np.uint8), []
        for k, pic in enumerate(c["pics"]):
            s = JR.encode(pic, c["q"], c["rr"])
            want_sizes.append(len(s) if len(s) <= c["slot"] else 0)
            if want_sizes[-1]:
                want[c["off"] + k * c["stride"]:c["off"] + k * c["stride"] + len(s)] = np.frombuffer(s, np.uint8)
        overflowed += want_sizes.count(0)
        assert list(sizes) == want_sizes, (i, list(sizes), want_sizes)
        assert np.array_equal(got, want), "case %d: %d bytes differ" % (i, int((got != want).sum()))
    assert pos == out.size and overflowed == 1


def test_the_kernels_run_on_the_host_equal_the_reference(tmp_path):
    """tests/cpp/jpeg_kernel_host.cpp: csrc/rip_jpeg.hip compiled as host code with the toolchain's clang++, every thread of the four
    launchers' grids run in turn from exactly sized sources and scratch into destinations with sentinels."""
    run_host_kernels(tmp_path, sanitize=False)


def test_the_kernels_run_on_the_host_under_asan_and_ubsan(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined: no access leaves a buffer, no wide access is misaligned."""
    run_host_kernels(tmp_path, sanitize=True)
