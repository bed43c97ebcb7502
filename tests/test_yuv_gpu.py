"""The YUV 4:2:0 output formats on the GPU (include/rip.h rip_set_output_yuv_matrix; csrc/rip_yuv.hip): every delivered byte at
tolerance 0 against tests/yuv_reference.py of the image a twin handle delivers under "native" with the same window, size, fit and pad
-- the image the rest of the suite pins against the oracle -- and every byte around the delivered rows against a sentinel.

Shapes: widths 2 .. 18 (whole lanes of 8 columns and the ragged ends 2, 4, 6), 510 and 514 -- one on each side of the 512 columns one
workgroup spans (rip_yuv.hpp kYuvPxPerBlockX = 64 lanes x 8 columns) -- and heights 2, 4, 6 (less than the 4 row pairs of a workgroup,
and more) and 66 (several workgroups in y)."""
import ctypes as C

import numpy as np
import pytest

import heads_cases as HC
import packed_reference as PR
import yuv_reference as Y
import yuv_variant_cases as YV
from helpers import cfg, configure
from raw_image_pipeline_amd import RawImagePipeline, synth
from raw_image_pipeline_amd import pipeline as P

gpu = pytest.mark.gpu
SENTINEL = 0xA5
WIDTHS = (2, 4, 6, 8, 10, 14, 16, 18, 510, 514)
HEIGHTS = (2, 4, 6, 66)
BAYER = "bayer_rggb8"


def plain_pipe(device=0):
    p = RawImagePipeline(False, "", "", "", device=device)
    configure(p, cfg())
    return p


def bgr_frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def raw_apply_device(pipe, frames_t, enc, ptr, step, frame_stride):
    n, rows, cols = frames_t.shape[:3]
    cn = frames_t.shape[3] if frames_t.dim() == 4 else 1
    st = pipe._lib.rip_apply_device(pipe._h, C.c_void_p(frames_t.data_ptr()), C.c_size_t(0), C.c_size_t(0), int(n), int(rows), int(cols), int(cn),
                                    enc.encode(), C.c_void_p(ptr), C.c_size_t(step), C.c_size_t(frame_stride), None, None)
    return st, pipe._lib.rip_last_error(pipe._h).decode()


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("matrix", Y.NAMES)
@pytest.mark.parametrize("fmt", Y.FORMATS)
def test_shapes(rip_lib, fmt, matrix):
    import torch
    p = plain_pipe()
    p.set_output_format(fmt)
    p.set_output_yuv_matrix(matrix)
    for w in WIDTHS:
        for h in HEIGHTS:
            e = bgr_frames(2, h, w, 1000 * w + h)
            e[1, :2, :2] = [255, 0, 0] if (w + h) % 4 else [0, 0, 255]          # where the full-range min binds
            with p.launch_log() as log:
                out = p.apply_device(torch.from_numpy(e).cuda(), "bgr8")
                torch.cuda.synchronize()
            assert [n for n in log.names() if "yuv420" in n or "output_convert" in n] == [YV.CASES[Y.FORMATS.index(fmt)].name]
            assert tuple(out.shape) == (2, 3 * h // 2, w) and out.dtype == torch.uint8 and p.last_encoding == fmt
            got = out.cpu().numpy()
            for k in range(2):
                assert np.array_equal(got[k], Y.convert(e[k], fmt, matrix)), (fmt, matrix, w, h, k)


def test_the_identity_chain_is_the_identity_the_shapes_rely_on():
    """test_shapes feeds bgr8 frames through a handle with every stage off; that this delivers the frame itself under "native" is what
    tests/test_golden.py and the fuzz of the suite pin.  Here only: the plan of such a handle has no stage (CPU)."""
    p = plain_pipe(device=-1)
    assert p.query_output(6, 10, 3, "bgr8") == (6, 10, 3, "bgr8")


@gpu
def test_native_of_a_plain_bgr_frame_is_the_frame(rip_lib):
    import torch
    e = bgr_frames(1, 6, 18, 5)
    out = plain_pipe().apply_device(torch.from_numpy(e).cuda(), "bgr8")
    assert np.array_equal(out.cpu().numpy(), e)


# ---- destinations --------------------------------------------------------------------------------------------------------------------
def destinations(fmt, w):
    """(name, base offset, pitch, extra frame gap, frames)"""
    return [("tight", 0, 0, 0, 1), ("p16", 0, (w + 15) // 16 * 16 + 16, 32, 1),
            ("odd" if fmt == "nv12" else "even_not_4", 0, w + 3 if fmt == "nv12" else (w + 2 if (w + 2) % 4 else w + 6), 0, 1),
            ("base_off_1", 1, 0, 0, 1), ("batch_of_3", 3, w + 6, 7, 3)]


@gpu
@pytest.mark.parametrize("fmt", Y.FORMATS)
@pytest.mark.parametrize("size", [(18, 6), (16, 4), (514, 6), (14, 66)])
def test_destinations_keep_every_byte_they_do_not_own(rip_lib, fmt, size):
    import torch
    w, h = size
    p = plain_pipe()
    p.set_output_format(fmt)
    p.set_output_yuv_matrix("bt709")
    for name, off, pitch, gap, n in destinations(fmt, w):
        e = bgr_frames(n, h, w, 77 + w + n)
        step = pitch or w
        stride = step * (3 * h // 2) + gap
        total = off + stride * n + 16
        backing = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
        tight = pitch == 0 and n == 1
        st, msg = raw_apply_device(p, torch.from_numpy(e).cuda(), "bgr8", backing.data_ptr() + off, 0 if tight else step, 0 if tight or n == 1 else stride)
        assert st == P.RIP_OK, (name, msg)
        torch.cuda.synchronize()
        want = np.full(total, SENTINEL, np.uint8)
        for k in range(n):
            frame = Y.pitched(e[k], fmt, "bt709", step, total=stride)
            own = Y.pitched(np.zeros_like(e[k]), fmt, "bt601_full", step, fill=1, total=stride) != 1
            want[off + k * stride:off + (k + 1) * stride][own] = frame[own]
        got = backing.cpu().numpy()
        assert np.array_equal(got, want), "%s %s %dx%d: %d bytes differ" % (fmt, name, w, h, int((got != want).sum()))


# ---- behind the pipeline ---------------------------------------------------------------------------------------------------------------
CONTEXTS = {
    "full_chain_undistorted": ("und200", HC.Head()),
    "linear": ("bayer136", HC.Head(size=(64, 48))),
    "area": ("bayer136", HC.Head(size=(50, 30), interp="area")),
    "cubic_aa": ("und200", HC.Head(size=(96, 64), interp="cubic_aa", fit="crop")),
    "window": ("bayer136", HC.Head(roi=(8, 4, 64, 32))),
    "letterbox_grey": ("bayer136", HC.Head(size=(64, 48), fit="letterbox")),
    "letterbox_colour": ("und200", HC.Head(size=(64, 64), fit="letterbox", interp="area", pad=(3, 128, 250))),
}


def twin_pair(frame, head, fmt, matrix):
    pipes = []
    for f in ("native", fmt):
        p = RawImagePipeline(False, "", "", "", device=0)
        HC.configure_pipeline(p, frame)
        HC.apply_head(p, head._replace(format=f))
        p.set_output_yuv_matrix(matrix)
        pipes.append(p)
    return pipes


@gpu
@pytest.mark.parametrize("fmt", Y.FORMATS)
@pytest.mark.parametrize("name", sorted(CONTEXTS))
def test_behind_the_pipeline(rip_lib, name, fmt):
    import torch
    frame, head = CONTEXTS[name]
    matrix = Y.NAMES[sorted(CONTEXTS).index(name) % 4]
    twin, p = twin_pair(frame, head, fmt, matrix)
    enc = HC.FRAMES[frame].encoding
    t = torch.from_numpy(HC.gen_frames(frame, 2, seed=3)).cuda()
    want = twin.apply_device(t, enc).cpu().numpy()
    got = p.apply_device(t, enc).cpu().numpy()
    assert got.shape == (2, 3 * want.shape[1] // 2, want.shape[2])
    for k in range(2):
        assert np.array_equal(got[k], Y.convert(want[k], fmt, matrix)), (name, fmt, k)
    if name.startswith("letterbox"):          # the pad colour lands in all three planes
        y, cb, cr = Y.planes(want[0], matrix)
        b, g, r = head.pad
        py, pcb, pcr = Y.planes(np.broadcast_to(np.array([b, g, r], np.uint8), (2, 2, 3)).copy(), matrix)
        gy, gcb, gcr = P.yuv_planes(got[0], fmt)
        assert gy[0, 0] == py[0, 0] and gcb[0, 0] == pcb[0, 0] and gcr[0, 0] == pcr[0, 0]
        if (b, g, r) == (114, 114, 114):
            assert (int(gcb[0, 0]), int(gcr[0, 0])) == (128, 128)


@gpu
@pytest.mark.parametrize("fmt", Y.FORMATS)
def test_behind_mht_and_a_packed_12_bit_frame(rip_lib, fmt):
    w, h = 136, 72
    layout = next(l for l in PR.BITS if PR.BITS[l] == 12)
    enc = PR.enc("rggb", layout)
    samples = np.random.default_rng(9).integers(0, 4096, (h, w)).astype(np.uint16)
    packed = PR.pack(samples, layout)
    outs = []
    for f in ("native", fmt):
        p = RawImagePipeline(False, "", "", "", device=0)
        configure(p, cfg(gamma=True))
        p.set_debayer_method("mht")
        p.set_output_format(f)
        p.set_output_yuv_matrix("bt709_full")
        outs.append(p.process(packed, enc, width=w))
    assert outs[0].shape == (h, w, 3) and np.array_equal(outs[1], Y.convert(outs[0], fmt, "bt709_full"))


# ---- heads -----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_an_nv12_head_beside_a_direct_native_head_and_a_tensor_head(rip_lib):
    import torch
    frame = "und208"          # 624 bytes per row of F: the tight identity head is written directly
    heads = (HC.IDENTITY, HC.Head(format="nv12", size=(64, 48), fit="letterbox", pad=(3, 128, 250)), HC.LETTERBOX_F16)
    enc = HC.FRAMES[frame].encoding
    p = RawImagePipeline(False, "", "", "", device=0)
    HC.configure_pipeline(p, frame)
    HC.configure_heads(p, heads)
    p.select_output_head(1)
    p.set_output_yuv_matrix("bt709")
    p.select_output_head(0)
    t = torch.from_numpy(HC.gen_frames(frame, 2, seed=1)).cuda()
    with p.launch_log() as log:
        outs = p.apply_device_heads(t, enc)
        torch.cuda.synchronize()
    assert p.debug_output_head_info(0)[1] == 1 and p.debug_output_head_info(1)[1:] == (0, 0)
    names = log.names()
    assert [n for n in names if "yuv420" in n] == ["yuv420_kernel<true>"]
    # the launches in order: ... chain, head 1's resize + pad + yuv, head 2's resize + pad + converter: one converter, and it is head 2's
    assert [n for n in names if "output_convert_kernel" in n] == ["output_convert_kernel<RgbChwF16>"]
    assert names.index("yuv420_kernel<true>") < names.index("output_convert_kernel<RgbChwF16>")
    for k, head in enumerate(heads):
        twin = RawImagePipeline(False, "", "", "", device=0)
        HC.configure_pipeline(twin, frame)
        HC.apply_head(twin, head._replace(format="native") if k == 1 else head)
        want = twin.apply_device(t, enc).cpu()
        if k == 1:
            for i in range(2):
                assert np.array_equal(outs[1][i].cpu().numpy(), Y.convert(want[i].numpy(), "nv12", "bt709"))
        else:
            assert torch.equal(outs[k].cpu(), want), k


# ---- host paths ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fmt", Y.FORMATS)
def test_host_paths(rip_lib, fmt):
    frame = "bayer136"
    enc = HC.FRAMES[frame].encoding
    frames = HC.gen_frames(frame, 3, seed=4)
    twin, p = twin_pair(frame, HC.Head(), fmt, "bt601")
    wants = [Y.convert(twin.process(f, enc), fmt, "bt601") for f in frames]
    h, w = 72, 136
    got = p.process(frames[0], enc)
    assert got.shape == (3 * h // 2, w) and got.dtype == np.uint8 and np.array_equal(got, wants[0]) and p.last_encoding == fmt
    assert np.array_equal(p.apply(frames[1].copy(), enc), wants[1])
    tickets = [p.submit(f, enc) for f in frames]
    for tk, want in zip(tickets, wants):
        assert np.array_equal(p.collect(tk), want)
    out = P.host_alloc((3 * h // 2, w))          # rip_submit_to: downloaded straight into the caller's page-locked array
    tk = p.submit(frames[2], enc, out=out)
    p.collect(tk)
    assert np.array_equal(out, wants[2])
    p.set_output_heads(2)
    res = p.apply_heads(frames[0], enc)
    assert np.array_equal(res[0], wants[0]) and res[1].shape == (h, w, 3)
    y, cb, cr = P.yuv_planes(got, fmt)
    ry, rcb, rcr = Y.planes(twin.process(frames[0], enc), "bt601")
    assert np.array_equal(y, ry) and np.array_equal(cb, rcb) and np.array_equal(cr, rcr)


# ---- ccc, refusals, masks --------------------------------------------------------------------------------------------------------------
@gpu
def test_ccc_sequence_with_a_refused_frame_in_between(rip_lib):
    pipes = []
    for f in ("native", "nv12"):
        p = RawImagePipeline(False, "", "", "", device=0)
        p.set_ccc_model(*synth.ccc_model())
        p.set_ccc_kalman_model(1.0, 10.0)
        configure(p, cfg(wb=True, wb_method="ccc", wb_bright=0.8, wb_dark=0.2, wb_temporal=True, gamma=True, gamma_k=0.9))
        p.reset_white_balance_temporal_consistency()
        p.set_output_format(f)
        pipes.append(p)
    twin, p = pipes
    frames = [synth.gen_frame(136, 72, BAYER, seed=20 + i) for i in range(4)]
    odd = synth.gen_frame(135, 71, BAYER, seed=99)
    for i, f in enumerate(frames):
        want = twin.process(f, BAYER)
        assert np.array_equal(p.process(f, BAYER), Y.convert(want, "nv12", "bt601")), i
        assert np.array_equal(p.get_ccc_track(1), twin.get_ccc_track(1)), i
        if i == 1:          # refused before anything is enqueued: the track is where it was
            before = p.get_ccc_track(1).copy()
            with pytest.raises(ValueError, match="even width and height.*135 x 71"):
                p.process(odd, BAYER)
            assert np.array_equal(p.get_ccc_track(1), before)


@gpu
def test_refusals_of_the_frame_calls(rip_lib):
    import torch
    e = torch.from_numpy(bgr_frames(1, 6, 18, 1)).cuda()
    backing = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    p = plain_pipe()
    p.set_output_format("i420")
    st, msg = raw_apply_device(p, e, "bgr8", backing.data_ptr(), 19, 0)
    assert st == P.RIP_ERR_INVALID_ARGUMENT and "even row pitch" in msg
    st, msg = raw_apply_device(p, e, "bgr8", backing.data_ptr(), 17, 0)
    assert st == P.RIP_ERR_INVALID_ARGUMENT and "smaller than a row" in msg
    st, msg = raw_apply_device(p, e, "bgr8", backing.data_ptr(), 20, 20 * 9 - 1)
    assert st == P.RIP_ERR_INVALID_ARGUMENT and "frame stride" in msg
    p.set_output_format("nv12")
    st, msg = raw_apply_device(p, e, "bgr8", backing.data_ptr(), 19, 0)          # an odd pitch is fine under nv12
    assert st == P.RIP_OK, msg
    for shape in ((1, 5, 18, 3), (1, 6, 17, 3)):
        st, msg = raw_apply_device(p, torch.zeros(shape, dtype=torch.uint8, device="cuda"), "bgr8", backing.data_ptr(), 0, 0)
        assert st == P.RIP_ERR_INVALID_ARGUMENT and "even width and height" in msg
    st, msg = raw_apply_device(p, torch.zeros((1, 6, 18), dtype=torch.uint8, device="cuda"), "mono8", backing.data_ptr(), 0, 0)
    assert st == P.RIP_ERR_INVALID_ARGUMENT and "three-channel" in msg
    torch.cuda.synchronize()
    p.set_output_format("native")
    p.set_output_heads(2)
    p.select_output_head(1)
    p.set_output_format("i420")
    with pytest.raises(ValueError, match="output head 1: .*even width and height"):
        p.apply_device_heads(torch.zeros((1, 5, 18, 3), dtype=torch.uint8, device="cuda"), "bgr8")


@gpu
def test_the_mask_of_a_yuv_head_is_the_pictures(rip_lib):
    frame, head = "und200", HC.Head(size=(64, 64), fit="letterbox")
    twin, p = twin_pair(frame, head, "i420", "bt601")
    f = HC.FRAMES[frame]
    for q in (twin, p):
        q.set_rect_mask("valid")
    want = twin.get_output_mask(f.size[1], f.size[0], 1, f.encoding)
    got = p.get_output_mask(f.size[1], f.size[0], 1, f.encoding)
    assert got.shape == (64, 64) and np.array_equal(got, want) and 0 < int((got == 255).sum()) < got.size


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------------
N_FUZZ = 30
FUZZ_SEED = 4200
FUZZ_FRAMES = ("bayer136", "und200")


def draw(rng):
    frame = FUZZ_FRAMES[int(rng.integers(2))]
    fmt, matrix = Y.FORMATS[int(rng.integers(2))], Y.NAMES[int(rng.integers(4))]
    resized = rng.integers(4) != 0
    size = (int(rng.integers(1, 120)) * (1 if rng.integers(8) == 0 else 2), int(rng.integers(1, 80)) * 2) if resized else (0, 0)
    interp = ("linear", "area", "linear_aa", "cubic_aa")[int(rng.integers(4))]
    fit = ("stretch", "letterbox", "crop")[int(rng.integers(3))]
    roi = (2 * int(rng.integers(0, 20)), int(rng.integers(0, 10)), 2 * int(rng.integers(8, 40)), 2 * int(rng.integers(8, 30))) if rng.integers(3) == 0 else (0, 0, 0, 0)
    pad = tuple(int(v) for v in rng.integers(0, 256, 3))
    pitch = ("tight", "p16", "plus6", "odd")[int(rng.integers(4))]
    return frame, fmt, matrix, HC.Head(size=size, interp=interp, fit=fit, roi=roi, pad=pad), pitch


def fuzz_configs():
    """N_FUZZ configurations the CPU rules accept, from one seeded stream: a drawn one is discarded only when rip_query_output refuses
    it on a handle without a device (an odd delivered size, an area upscale, a window outside F) or when it asks for an odd pitch under i420."""
    rng = np.random.default_rng(FUZZ_SEED)
    probe = RawImagePipeline(False, "", "", "", device=-1)
    accepted, drawn = [], 0
    while len(accepted) < N_FUZZ and drawn < 400:
        c = draw(rng)
        drawn += 1
        frame, fmt, matrix, head, pitch = c
        if fmt == "i420" and pitch == "odd":
            continue
        HC.configure_pipeline(probe, frame)
        HC.apply_head(probe, head._replace(format=fmt))
        f = HC.FRAMES[frame]
        try:
            probe.query_output(f.size[1], f.size[0], 1, f.encoding)
        except ValueError:
            continue
        accepted.append(c)
    return accepted, drawn


def test_the_fuzz_draws_what_it_claims(rip_lib):
    accepted, drawn = fuzz_configs()
    assert len(accepted) == N_FUZZ and drawn > N_FUZZ          # some were refused by the CPU rules, and 30 accepted remain
    assert {c[1] for c in accepted} == set(Y.FORMATS) and {c[2] for c in accepted} == set(Y.NAMES)
    assert {c[3].interp for c in accepted if c[3].size != (0, 0)} == {"linear", "area", "linear_aa", "cubic_aa"}
    assert {c[3].fit for c in accepted if c[3].size != (0, 0)} == {"stretch", "letterbox", "crop"}
    assert {c[4] for c in accepted} == {"tight", "p16", "plus6", "odd"}
    assert any(c[3].roi != (0, 0, 0, 0) for c in accepted) and any(c[3].size == (0, 0) for c in accepted)


@gpu
def test_fuzz(rip_lib):
    import torch
    accepted, _ = fuzz_configs()
    assert len(accepted) >= N_FUZZ
    inputs = {frame: torch.from_numpy(HC.gen_frames(frame, 2, seed=8)).cuda() for frame in FUZZ_FRAMES}
    for i, (frame, fmt, matrix, head, pitch) in enumerate(accepted):
        twin, p = twin_pair(frame, head, fmt, matrix)
        enc = HC.FRAMES[frame].encoding
        t = inputs[frame]
        want = twin.apply_device(t, enc).cpu().numpy()
        h, w = want.shape[1:3]
        step = {"tight": w, "p16": (w + 15) // 16 * 16 + 16, "plus6": w + 6, "odd": w + 3}[pitch]
        stride = step * (3 * h // 2) + (0 if pitch == "tight" else 10)
        backing = torch.full((1 + stride * 2 + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        st, msg = raw_apply_device(p, t, enc, backing.data_ptr() + 1, 0 if pitch == "tight" else step, 0 if pitch == "tight" else stride)
        assert st == P.RIP_OK, (i, msg)
        torch.cuda.synchronize()
        expect = np.full(backing.numel(), SENTINEL, np.uint8)
        for k in range(2):
            block = Y.pitched(want[k], fmt, matrix, step, total=stride)
            own = Y.pitched(np.zeros_like(want[k]), fmt, "bt601_full", step, fill=1, total=stride) != 1
            expect[1 + k * stride:1 + (k + 1) * stride][own] = block[own]
        got = backing.cpu().numpy()
        assert np.array_equal(got, expect), "configuration %d %r: %d bytes differ" % (i, (frame, fmt, matrix, head, pitch), int((got != expect).sum()))
