"""The output format "jpeg" on the GPU (include/rip.h rip_set_output_jpeg; csrc/rip_jpeg.hip): every delivered byte and every stream
length at tolerance 0 against tests/jpeg_reference.py's ``encode`` of the picture a twin handle delivers under "native" with the same
window, size, fit and pad -- the image the rest of the suite pins against the oracle -- and every byte of a slot behind its stream,
between slots and around them against a sentinel.

Shapes: one block and one MCU (8 x 8, 16 x 16), extension on either axis (17 x 9, 9 x 17, 1 x 1), MCU rows of more than 64 blocks
(colour 208 x 16: 78, grey 520 x 8: 65 -- more lanes than one workgroup of the transform has), 18 restart intervals (grey 8 x 144),
which wrap RSTm, and 2100 rows of grey for more intervals than one workgroup of the sizing and writing passes has."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import heads_cases as HC
import jpeg_reference as JR
from helpers import cfg, configure
from raw_image_pipeline_amd import RawImagePipeline, synth
from raw_image_pipeline_amd import pipeline as P
from test_cpp_facade import BRANCHES, run_env

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
BAYER = "bayer_rggb8"


def plain_pipe(quality=90, restart_rows=1, device=0):
    """Every stage off: a bgr8 or mono8 frame is its own "native" picture (tests/test_yuv_gpu.py pins that)."""
    p = RawImagePipeline(False, "", "", "", device=device)
    configure(p, cfg())
    p.set_output_format("jpeg")
    p.set_output_jpeg(quality, restart_rows)
    return p


def picture(kind, h, w, channels, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        pic = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    elif kind == "flat":
        pic = np.full((h, w, channels), rng.integers(0, 256, channels), np.uint8)
    elif kind == "gradient":
        g = (np.arange(w)[None, :] * 3 + np.arange(h)[:, None] * 2) % 256
        pic = np.stack([g, 255 - g, g // 2][:channels], -1).astype(np.uint8)
    else:  # 0 / 255 checkerboard: the largest categories and many 0xFF bytes
        g = (np.indices((h, w)).sum(0) % 2) * 255
        pic = np.repeat(g[..., None], channels, 2).astype(np.uint8)
    return np.ascontiguousarray(pic[..., 0] if channels == 1 else pic)


def raw_apply_device(pipe, frames_t, enc, ptr, step, frame_stride):
    n, rows, cols = frames_t.shape[:3]
    cn = frames_t.shape[3] if frames_t.dim() == 4 else 1
    st = pipe._lib.rip_apply_device(pipe._h, C.c_void_p(frames_t.data_ptr()), C.c_size_t(0), C.c_size_t(0), int(n), int(rows), int(cols), int(cn),
                                    enc.encode(), C.c_void_p(ptr), C.c_size_t(step), C.c_size_t(frame_stride), None, None)
    return st, pipe._lib.rip_last_error(pipe._h).decode()


def check_slots(got, sizes, pictures, quality, restart_rows, fill=None):
    """got [n, slot]: frame k holds encode(pictures[k]) and, with `fill`, that byte behind it; returns the streams."""
    slot = got.shape[1]
    streams = [JR.encode(pic, quality, restart_rows) for pic in pictures]
    assert list(sizes) == [len(s) if len(s) <= slot else 0 for s in streams]
    for k, s in enumerate(streams):
        if len(s) <= slot:
            assert got[k, :len(s)].tobytes() == s, "frame %d: the stream differs" % k
        if fill is not None:
            assert (got[k, len(s) if len(s) <= slot else 0:] == fill).all(), "frame %d: bytes behind the stream were written" % k
    return streams


# (h, w, channels, quality, restart_rows, contents)
SHAPES = [(8, 8, 1, 90, 1, "noise"), (8, 8, 3, 90, 1, "noise"), (16, 16, 3, 90, 1, "noise"), (16, 16, 1, 50, 2, "gradient"),
          (9, 17, 3, 90, 1, "noise"), (17, 9, 3, 50, 2, "gradient"), (9, 17, 1, 90, 1, "noise"), (17, 9, 1, 100, 64, "checker"),
          (1, 1, 3, 90, 1, "noise"), (1, 1, 1, 1, 1, "noise"), (16, 208, 3, 90, 1, "noise"), (8, 520, 1, 90, 1, "noise"),
          (144, 8, 1, 90, 1, "noise"), (40, 56, 3, 100, 2, "checker"), (40, 56, 1, 1, 1, "checker"), (24, 24, 3, 1, 64, "flat"),
          (33, 47, 3, 100, 1, "gradient"), (48, 40, 3, 50, 64, "noise"), (2100, 24, 1, 90, 1, "gradient")]


@gpu
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "%dx%dx%d_q%d_r%d_%s" % c)
def test_shapes(rip_lib, case):
    import torch
    h, w, ch, quality, rr, kind = case
    p = plain_pipe(quality, rr)
    pics = [picture(kind, h, w, ch, 100 + k) for k in range(2)]
    slot = JR.default_slot(h, w, ch, rr)
    enc = "mono8" if ch == 1 else "bgr8"
    assert p.query_output(h, w, ch, enc) == (1, slot, 1, "jpeg") and p.query_output_bytes(h, w, ch, enc) == (slot, 1, False)
    with p.launch_log() as log:
        out = p.apply_device(torch.from_numpy(np.stack(pics)).cuda(), enc)
        sizes = p.jpeg_sizes()
    colour = "true" if ch == 3 else "false"
    assert [n for n in log.names() if "jpeg" in n] == ["jpeg_transform_kernel<%s>" % colour, "jpeg_size_kernel", "jpeg_scan_kernel", "jpeg_write_kernel"]
    assert tuple(out.shape) == (2, slot) and out.dtype == torch.uint8 and p.last_encoding == "jpeg"
    streams = check_slots(out.cpu().numpy(), sizes, pics, quality, rr)
    assert all(0 < len(s) <= slot for s in streams)
    assert P.jpeg_streams(out, sizes) == streams
    if (h, w) == (144, 8):
        assert JR.decode_coefficients(streams[0])["restarts"] == [k % 8 for k in range(17)]


def overflow_pictures():
    noisy = picture("noise", 32, 32, 3, 7)
    return [picture("flat", 32, 32, 3, 1), noisy, picture("gradient", 32, 32, 3, 2)]


def test_the_overflow_picture_overflows_the_default_slot():
    flat, noisy, grad = (len(JR.encode(pic, 100, 1)) for pic in overflow_pictures())
    slot = JR.default_slot(32, 32, 3, 1)
    assert noisy > slot and flat <= slot and grad <= slot and noisy <= 8000


@gpu
def test_a_frame_that_overflows_its_slot_is_left_alone_and_its_neighbours_are_not(rip_lib):
    import torch
    pics = overflow_pictures()
    p = plain_pipe(100, 1)
    slot = JR.default_slot(32, 32, 3, 1)
    out = torch.full((3, slot), SENTINEL, dtype=torch.uint8, device="cuda")
    assert p.apply_device(torch.from_numpy(np.stack(pics)).cuda(), "bgr8", out=out) is out
    sizes = p.jpeg_sizes()
    assert sizes[1] == 0 and sizes[0] > 0 and sizes[2] > 0
    check_slots(out.cpu().numpy(), sizes, pics, 100, 1, fill=SENTINEL)
    # the same picture in a slot the caller chose: a wider tensor is a larger slot
    big = torch.full((3, 8000), SENTINEL, dtype=torch.uint8, device="cuda")
    p.apply_device(torch.from_numpy(np.stack(pics)).cuda(), "bgr8", out=big)
    sizes = p.jpeg_sizes()
    assert (sizes > 0).all() and sizes[1] > slot
    check_slots(big.cpu().numpy(), sizes, pics, 100, 1, fill=SENTINEL)


@gpu
@pytest.mark.parametrize("layout", [("base_1", 1, 0, 0), ("base_3_gap_5", 3, 0, 5), ("slot_plus_7", 2, 7, 0), ("small_slot", 5, None, 13)])
def test_destinations_keep_every_byte_they_do_not_own(rip_lib, layout):
    import torch
    name, off, slot_delta, gap = layout
    for ch, (h, w) in ((3, (24, 40)), (1, (17, 33))):
        p = plain_pipe(90, 2)
        pics = [picture(("noise", "flat", "gradient")[k], h, w, ch, 40 + k) for k in range(3)]
        # small_slot: one byte less than the noise frame's stream needs -- it overflows, its neighbours fit
        slot = JR.default_slot(h, w, ch, 2) + slot_delta if slot_delta is not None else len(JR.encode(pics[0], 90, 2)) - 1
        stride = slot + gap
        total = off + stride * 3 + 16
        backing = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
        st, msg = raw_apply_device(p, torch.from_numpy(np.stack(pics)).cuda(), "mono8" if ch == 1 else "bgr8", backing.data_ptr() + off,
                                   slot if slot_delta or gap else 0, stride if gap else 0)
        assert st == P.RIP_OK, (name, msg)
        sizes = p.jpeg_sizes()
        want = np.full(total, SENTINEL, np.uint8)
        want_sizes = []
        for k, pic in enumerate(pics):
            s = JR.encode(pic, 90, 2)
            want_sizes.append(len(s) if len(s) <= slot else 0)
            if len(s) <= slot:
                want[off + k * stride:off + k * stride + len(s)] = np.frombuffer(s, np.uint8)
        got = backing.cpu().numpy()
        assert list(sizes) == want_sizes and np.array_equal(got, want), "%s: %d bytes differ" % (name, int((got != want).sum()))
        if name == "small_slot":
            assert 0 in want_sizes and any(want_sizes)


# ---- behind the pipeline ---------------------------------------------------------------------------------------------------------------
CONTEXTS = {
    "resize_linear": ("bayer136", HC.Head(size=(63, 47))),
    "window": ("bayer136", HC.Head(roi=(8, 4, 61, 31))),
    "letterbox_colour": ("und200", HC.Head(size=(64, 64), fit="letterbox", interp="area", pad=(3, 128, 250))),
    "undistorted_200": ("und200", HC.Head()),
    "mono_camera": ("mono65", HC.Head()),
    "mono_camera_resized": ("mono65", HC.Head(size=(40, 21), interp="area")),
}


def twin_pair(frame, head, quality=90, restart_rows=1):
    pipes = []
    for f in ("native", "jpeg"):
        p = RawImagePipeline(False, "", "", "", device=0)
        HC.configure_pipeline(p, frame)
        HC.apply_head(p, head._replace(format=f))
        p.set_output_jpeg(quality, restart_rows)
        pipes.append(p)
    return pipes


@gpu
@pytest.mark.parametrize("name", sorted(CONTEXTS))
def test_behind_the_pipeline(rip_lib, name):
    import torch
    frame, head = CONTEXTS[name]
    quality, rr = (75, 2) if "letterbox" in name else (90, 1)
    twin, p = twin_pair(frame, head, quality, rr)
    enc = HC.FRAMES[frame].encoding
    t = torch.from_numpy(HC.gen_frames(frame, 2, seed=3)).cuda()
    want = twin.apply_device(t, enc).cpu().numpy()
    out = p.apply_device(t, enc)
    check_slots(out.cpu().numpy(), p.jpeg_sizes(), list(want), quality, rr)
    f = HC.FRAMES[frame]
    assert p.get_output_window(f.size[1], f.size[0], 1, f.encoding) == twin.get_output_window(f.size[1], f.size[0], 1, f.encoding)


@gpu
def test_behind_the_full_chain_with_undistortion_at_136_x_72(rip_lib):
    import torch
    pipes = []
    for f in ("native", "jpeg"):
        p = RawImagePipeline(False, "", "", "", device=0)
        configure(p, cfg(wb=True, wb_method="grey_world", cc=True, gamma=True, vig=True, ce=True, ce_sat=1.2, undistort=True, cam=synth.camera_model(136, 72)))
        p.set_output_format(f)
        pipes.append(p)
    twin, p = pipes
    t = torch.from_numpy(np.stack([synth.gen_frame(136, 72, BAYER, seed=50 + i) for i in range(2)])).cuda()
    want = twin.apply_device(t, BAYER).cpu().numpy()
    assert want.shape == (2, 72, 136, 3)
    check_slots(p.apply_device(t, BAYER).cpu().numpy(), p.jpeg_sizes(), list(want), 90, 1)
    for q in (twin, p):
        q.set_rect_mask("valid")
    assert np.array_equal(p.get_output_mask(72, 136, 1, BAYER), twin.get_output_mask(72, 136, 1, BAYER))


# ---- heads -----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_jpeg_head_beside_a_direct_native_head_and_a_tensor_head(rip_lib):
    import torch
    frame = "und208"          # 624 bytes per row of F: the tight identity head is written directly
    heads = (HC.IDENTITY, HC.Head(format="jpeg", size=(64, 48), fit="letterbox", pad=(3, 128, 250)), HC.LETTERBOX_F16)
    enc = HC.FRAMES[frame].encoding
    p = RawImagePipeline(False, "", "", "", device=0)
    HC.configure_pipeline(p, frame)
    HC.configure_heads(p, heads)
    p.select_output_head(1)
    p.set_output_jpeg(60, 2)
    p.select_output_head(0)
    t = torch.from_numpy(HC.gen_frames(frame, 2, seed=1)).cuda()
    with p.launch_log() as log:
        outs = p.apply_device_heads(t, enc)
        torch.cuda.synchronize()
    assert p.debug_output_head_info(0)[1] == 1 and p.debug_output_head_info(1)[1:] == (0, 0)          # never the head the chain writes
    names = log.names()
    assert [n for n in names if "jpeg" in n] == ["jpeg_transform_kernel<true>", "jpeg_size_kernel", "jpeg_scan_kernel", "jpeg_write_kernel"]
    assert names.index("jpeg_write_kernel") < names.index("output_convert_kernel<RgbChwF16>")
    assert len(p.jpeg_sizes()) == 0 and len(p.jpeg_sizes(head=1)) == 2 and p.get_selected_output_head() == 0
    for k, head in enumerate(heads):
        twin = RawImagePipeline(False, "", "", "", device=0)
        HC.configure_pipeline(twin, frame)
        HC.apply_head(twin, head._replace(format="native") if k == 1 else head)
        want = twin.apply_device(t, enc).cpu()
        if k == 1:
            check_slots(outs[1].cpu().numpy(), p.jpeg_sizes(head=1), list(want.numpy()), 60, 2)
        else:
            assert torch.equal(outs[k].cpu(), want), k


# ---- host paths ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_host_paths_and_the_ring_refusal(rip_lib):
    frame = "bayer136"
    enc = HC.FRAMES[frame].encoding
    frames = HC.gen_frames(frame, 2, seed=4)
    twin, p = twin_pair(frame, HC.Head(), 80, 3)
    wants = [JR.encode(twin.process(f, enc), 80, 3) for f in frames]
    got = p.process(frames[0], enc)
    assert got.dtype == np.uint8 and got.ndim == 1 and got.tobytes() == wants[0] and p.last_encoding == "jpeg"
    assert list(p.jpeg_sizes()) == [len(wants[0])]
    assert p.apply(frames[1].copy(), enc).tobytes() == wants[1]
    track = p.get_white_balance_info(1).copy()
    with pytest.raises(ValueError, match="jpeg.*ring"):
        p.submit(frames[0], enc)
    out = P.host_alloc((JR.default_slot(72, 136, 3, 3),))
    with pytest.raises(ValueError, match="jpeg.*ring"):
        p.submit(frames[0], enc, out=out)
    assert np.array_equal(p.get_white_balance_info(1), track)
    p.set_output_heads(2)
    res = p.apply_heads(frames[0], enc)
    assert res[0].tobytes() == wants[0] and res[1].shape == (72, 136, 3) and np.array_equal(res[1], twin.process(frames[0], enc))


# ---- a handle without jpeg, ccc, refusals ----------------------------------------------------------------------------------------------
@gpu
def test_a_handle_without_jpeg_launches_what_it_launched(rip_lib):
    import torch
    t = torch.from_numpy(HC.gen_frames("bayer136", 1, seed=2)).cuda()
    logs = {}
    for fmt in ("native", "rgb8", "nv12", "jpeg"):
        p = RawImagePipeline(False, "", "", "", device=0)
        HC.configure_pipeline(p, "bayer136")
        p.set_output_jpeg(30, 4)          # without effect under the other formats
        p.set_output_format(fmt)
        with p.launch_log() as log:
            p.apply_device(t, BAYER)
            torch.cuda.synchronize()
        logs[fmt] = log.names()
        assert len(p.jpeg_sizes()) == (1 if fmt == "jpeg" else 0)
    assert not [n for f in ("native", "rgb8", "nv12") for n in logs[f] if "jpeg" in n]
    assert logs["rgb8"][:-1] == logs["nv12"][:-1] == logs["jpeg"][:-4]          # the same chain in front, the encoder's four launches behind


@gpu
def test_ccc_sequence_with_a_refused_frame_in_between(rip_lib):
    import torch
    pipes = []
    for f in ("native", "jpeg"):
        p = RawImagePipeline(False, "", "", "", device=0)
        p.set_ccc_model(*synth.ccc_model())
        p.set_ccc_kalman_model(1.0, 10.0)
        configure(p, cfg(wb=True, wb_method="ccc", wb_bright=0.8, wb_dark=0.2, wb_temporal=True, gamma=True, gamma_k=0.9))
        p.reset_white_balance_temporal_consistency()
        p.set_output_format(f)
        pipes.append(p)
    twin, p = pipes
    frames = [synth.gen_frame(136, 72, BAYER, seed=20 + i) for i in range(4)]
    for i, f in enumerate(frames):
        want = twin.process(f, BAYER)
        assert p.process(f, BAYER).tobytes() == JR.encode(want, 90, 1), i
        assert np.array_equal(p.get_ccc_track(1), twin.get_ccc_track(1)), i
        if i == 1:          # refused before anything is enqueued: the track is where it was
            before = p.get_ccc_track(1).copy()
            small = torch.zeros((1, JR.HEADER_BYTES[3] + 1), dtype=torch.uint8, device="cuda")
            with pytest.raises(ValueError, match="smaller than the header and EOI"):
                p.apply_device(torch.from_numpy(f[None]).cuda(), BAYER, out=small)
            p.set_output_clahe(2.0, 4, 4)
            with pytest.raises(ValueError, match="does not take CLAHE"):
                p.process(f, BAYER)
            p.set_output_clahe(0.0, 0, 0)
            assert np.array_equal(p.get_ccc_track(1), before)


@gpu
def test_the_lengths_are_those_of_the_heads_last_frame_call(rip_lib):
    """rip_get_output_jpeg_sizes: empty before the first frame call, after a frame call that delivered another format from the head and
    for a head rip_set_output_heads has reset; a refused call leaves the lengths of the call before; a head that a heads call does not
    request keeps its own."""
    import torch
    p = plain_pipe(90, 1)
    pics = np.stack([picture("gradient", 24, 40, 3, k) for k in range(3)])
    t = torch.from_numpy(pics).cuda()
    assert len(p.jpeg_sizes()) == 0
    p.apply_device(t, "bgr8")
    want = [len(JR.encode(pic, 90, 1)) for pic in pics]
    assert list(p.jpeg_sizes()) == want
    with pytest.raises(ValueError, match="smaller than the header and EOI"):
        p.apply_device(t, "bgr8", out=torch.zeros((3, 100), dtype=torch.uint8, device="cuda"))
    assert list(p.jpeg_sizes()) == want
    p.apply_device(t[:1], "bgr8")
    assert list(p.jpeg_sizes()) == want[:1]
    p.set_output_format("rgb8")
    p.apply_device(t, "bgr8")
    assert len(p.jpeg_sizes()) == 0
    p.set_output_format("jpeg")
    p.set_output_heads(2)
    p.select_output_head(1)
    p.set_output_format("jpeg")
    p.apply_device_heads(t, "bgr8")
    assert list(p.jpeg_sizes(head=0)) == want and list(p.jpeg_sizes(head=1)) == want
    p.apply_device_heads(t[:2], "bgr8", heads=[0])          # head 1 is not requested: its last call stands
    assert list(p.jpeg_sizes(head=0)) == want[:2] and list(p.jpeg_sizes(head=1)) == want
    p.set_output_heads(1)
    p.set_output_heads(2)
    assert len(p.jpeg_sizes(head=1)) == 0 and list(p.jpeg_sizes(head=0)) == want[:2]
    assert p.process(pics[0], "bgr8").tobytes() == JR.encode(pics[0], 90, 1) and list(p.jpeg_sizes()) == want[:1]


# ---- the facade ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade_delivers_the_stream_and_its_length(tmp_path, rip_lib, branch):
    """tests/cpp/jpeg_test.cpp gpu: process() under "jpeg" and getOutputJpegSizes' two calls, count first and then fill, on real lengths."""
    exe = str(tmp_path / ("jpeg_test_" + branch.replace("-", "_")))
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror"] + BRANCHES[branch] + ["-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "jpeg_test.cpp"), "-o", exe, "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir,
           "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    w, h = 72, 40
    out_path = str(tmp_path / "out.bin")
    r = subprocess.run([exe, "gpu", str(w), str(h), out_path], capture_output=True, text=True, env=run_env(0))
    assert r.returncode == 0 and "jpeg gpu OK" in r.stdout, r.stdout + r.stderr
    blob = np.fromfile(out_path, np.uint8)
    native = blob[:w * h * 3].reshape(h, w, 3)
    count, size = blob[w * h * 3:w * h * 3 + 8].view(np.uint32)
    want = JR.encode(native, 85, 2)
    assert count == 1 and size == len(want) and blob[w * h * 3 + 8:].tobytes() == want


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------------
N_FUZZ = 30
FUZZ_SEED = 5100
FUZZ_FRAMES = ("bayer136", "und200", "mono65")


def draw(rng):
    frame = FUZZ_FRAMES[int(rng.integers(3))]
    resized = rng.integers(4) != 0
    size = (int(rng.integers(1, 120)), int(rng.integers(1, 80))) if resized else (0, 0)
    interp = ("linear", "area", "linear_aa", "cubic_aa")[int(rng.integers(4))]
    fit = ("stretch", "letterbox", "crop")[int(rng.integers(3))]
    roi = (int(rng.integers(0, 20)), int(rng.integers(0, 10)), int(rng.integers(8, 40)), int(rng.integers(8, 24))) if rng.integers(3) == 0 else (0, 0, 0, 0)
    pad = tuple(int(v) for v in rng.integers(0, 256, 3))
    quality = int((1, 25, 50, 75, 90, 95, 100)[int(rng.integers(7))])
    restart_rows = int((1, 1, 2, 3, 64)[int(rng.integers(5))])
    slot = ("default", "plus9", "large", "small")[int(rng.integers(4))]
    return frame, HC.Head(size=size, interp=interp, fit=fit, roi=roi, pad=pad), quality, restart_rows, slot, int(rng.integers(0, 8))


def fuzz_configs():
    """N_FUZZ configurations the CPU rules accept, from one seeded stream: a drawn one is discarded only when rip_query_output refuses
    it on a handle without a device (an area upscale, a window outside F, a factor beyond a filter's limit)."""
    rng = np.random.default_rng(FUZZ_SEED)
    probe = RawImagePipeline(False, "", "", "", device=-1)
    accepted, drawn = [], 0
    while len(accepted) < N_FUZZ and drawn < 400:
        c = draw(rng)
        drawn += 1
        HC.configure_pipeline(probe, c[0])
        HC.apply_head(probe, c[1]._replace(format="jpeg"))
        f = HC.FRAMES[c[0]]
        try:
            probe.query_output(f.size[1], f.size[0], 1, f.encoding)
        except ValueError:
            continue
        accepted.append(c)
    return accepted, drawn


def test_the_fuzz_draws_what_it_claims(rip_lib):
    accepted, drawn = fuzz_configs()
    assert len(accepted) == N_FUZZ and drawn > N_FUZZ
    assert {c[0] for c in accepted} == set(FUZZ_FRAMES) and {c[4] for c in accepted} == {"default", "plus9", "large", "small"}
    assert {c[3] for c in accepted} == {1, 2, 3, 64} and len({c[2] for c in accepted}) >= 6
    assert {c[1].fit for c in accepted if c[1].size != (0, 0)} == {"stretch", "letterbox", "crop"}
    assert any(c[1].roi != (0, 0, 0, 0) for c in accepted) and any(c[1].size == (0, 0) for c in accepted)


@gpu
def test_fuzz(rip_lib):
    import torch
    accepted, _ = fuzz_configs()
    assert len(accepted) >= N_FUZZ
    inputs = {frame: torch.from_numpy(HC.gen_frames(frame, 2, seed=8)).cuda() for frame in FUZZ_FRAMES}
    overflowed = 0
    for i, (frame, head, quality, rr, slot_kind, off) in enumerate(accepted):
        twin, p = twin_pair(frame, head, quality, rr)
        enc = HC.FRAMES[frame].encoding
        t = inputs[frame]
        want = twin.apply_device(t, enc).cpu().numpy()
        h, w = want.shape[1:3]
        ch = 1 if want.ndim == 3 else 3
        default = JR.default_slot(h, w, ch, rr)
        assert p.query_output(t.shape[1], t.shape[2], 1, enc)[1] == default
        streams = [JR.encode(pic, quality, rr) for pic in want]
        slot = {"default": default, "plus9": default + 9, "large": 2 * default + 1, "small": max(JR.HEADER_BYTES[ch] + 2, max(len(s) for s in streams) - 1)}[slot_kind]
        stride = slot + (0 if slot_kind == "default" else 11)
        backing = torch.full((off + stride * 2 + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        st, msg = raw_apply_device(p, t, enc, backing.data_ptr() + off, 0 if slot_kind == "default" else slot, 0 if slot_kind == "default" else stride)
        assert st == P.RIP_OK, (i, msg)
        sizes = p.jpeg_sizes()
        expect = np.full(backing.numel(), SENTINEL, np.uint8)
        want_sizes = [len(s) if len(s) <= slot else 0 for s in streams]
        overflowed += want_sizes.count(0)
        for k, s in enumerate(streams):
            if want_sizes[k]:
                expect[off + k * stride:off + k * stride + len(s)] = np.frombuffer(s, np.uint8)
        got = backing.cpu().numpy()
        assert list(sizes) == want_sizes, (i, list(sizes), want_sizes)
        assert np.array_equal(got, expect), "configuration %d %r: %d bytes differ" % (i, accepted[i], int((got != expect).sum()))
    assert overflowed > 0
