"""CLAHE on the GPU (include/rip.h rip_set_output_clahe; csrc/rip_clahe.hip): every delivered byte at tolerance 0 against
tests/clahe_reference.py applied to the picture rectangle of the image a twin handle delivers with CLAHE off -- the image the rest of
the suite pins against the oracle -- and every byte around the picture against that twin's bands or a sentinel.

Shapes (tests/clahe_cases.py): sizes whose axes divide by the tiles, do not, or only one of them does; tiles (1, 1), two-pixel tiles
under (16, 16), (3, 5), (16, 1); 1100 columns, more than one pass of a workgroup's 256 lanes x 4 pixels; 700 x 300 under (2, 1), where a
bin count of a tile of 105 000 pixels passes 65 535."""
import ctypes as C

import numpy as np
import pytest

import clahe_cases as CC
import clahe_reference as CL
import clahe_variant_cases as CV
import heads_cases as HC
from helpers import cfg, configure
from raw_image_pipeline_amd import RawImagePipeline, synth
from raw_image_pipeline_amd import pipeline as P

gpu = pytest.mark.gpu
SENTINEL = 0xA5
BAYER = "bayer_rggb8"
KERNELS = CV.LAUNCH_ORDER


def plain_pipe(device=0):
    p = RawImagePipeline(False, "", "", "", device=device)
    configure(p, cfg())
    return p


def raw_apply_device(pipe, frames_t, enc, ptr, step, frame_stride):
    n, rows, cols = frames_t.shape[:3]
    cn = frames_t.shape[3] if frames_t.dim() == 4 else 1
    st = pipe._lib.rip_apply_device(pipe._h, C.c_void_p(frames_t.data_ptr()), C.c_size_t(0), C.c_size_t(0), int(n), int(rows), int(cols), int(cn),
                                    enc.encode(), C.c_void_p(ptr), C.c_size_t(step), C.c_size_t(frame_stride), None, None)
    return st, pipe._lib.rip_last_error(pipe._h).decode()


def pictures(content, n, h, w, seed):
    return np.stack([CC.picture(content, h, w, seed=seed + k) for k in range(n)])


def expected(delivered, rect, clip, tiles):
    """The twin's delivered frames [n, H, W] with the reference on their picture rectangle."""
    return np.stack([CL.apply_to_delivered(f, rect, clip, *tiles) for f in delivered])


def deliver_into_layout(p, t, enc, want, layout):
    """Runs rip_apply_device of the frames `t` into a sentinel-filled block with the row padding, base offset and frame gap of
    `layout`, and compares every byte of the block: `want` [n, H, W] inside the rows, the sentinel everywhere else."""
    import torch
    pad, off, gap = layout
    n, h, w = want.shape
    step = w + pad
    stride = step * h + gap
    backing = torch.full((off + stride * n + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    tight = pad == 0 and gap == 0
    st, msg = raw_apply_device(p, t, enc, backing.data_ptr() + off, 0 if tight else step, 0 if tight else stride)
    assert st == P.RIP_OK, msg
    torch.cuda.synchronize()
    expect = np.full(backing.numel(), SENTINEL, np.uint8)
    for k in range(n):
        rows = np.lib.stride_tricks.as_strided(expect[off + k * stride:], (h, w), (step, 1))
        rows[...] = want[k]
    got = backing.cpu().numpy()
    assert np.array_equal(got, expect), "%d bytes differ" % int((got != expect).sum())


# ---- shapes, contents, clips, destinations: a mono frame under native without a resize, the path through the staging image ---------
ALL_SHAPES = CC.SHAPES + [CC.LARGE_SHAPE]


@gpu
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "%dx%d_%dx%d" % (s[0] + s[1]))
def test_out_of_place_shapes_contents_clips_and_destinations(rip_lib, shape):
    import torch
    (w, h), tiles = shape
    large = shape == CC.LARGE_SHAPE
    p = plain_pipe()
    k = ALL_SHAPES.index(shape)
    runs = [("flat", 3.0, 1, (0, 0, 0)), ("random", 40.0, 1, (1, 3, 0))] if large else [
        (CC.CONTENTS[(k + i) % 4], CC.CLIPS[(k + i) % 5], (1, 3, 5)[(k + i) % 3], CC.LAYOUTS[(k + i) % len(CC.LAYOUTS)]) for i in range(6)]
    for content, clip, n, layout in runs:
        pics = pictures(content, n, h, w, seed=100 * k)
        p.set_output_clahe(clip, *tiles)
        with p.launch_log() as log:
            deliver_into_layout(p, torch.from_numpy(pics).cuda(), "mono8", expected(pics, (0, 0, w, h), clip, tiles), layout)
        assert [name for name in log.names() if "clahe" in name] == KERNELS and log.names()[-2:] == KERNELS
    if large:
        assert np.bincount(pictures("flat", 1, h, w, seed=100 * k).ravel()).max() > 65535 * 2


@gpu
def test_a_plain_mono_frame_comes_back_as_it_is(rip_lib):
    """What the shapes above rely on: with every stage off and CLAHE off the delivered mono frame is the frame."""
    import torch
    pics = pictures("random", 2, 45, 67, seed=1)
    assert np.array_equal(plain_pipe().apply_device(torch.from_numpy(pics).cuda(), "mono8").cpu().numpy(), pics)


# ---- the in-place paths: behind a resize into the caller's buffer ----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", CC.SHAPES, ids=lambda s: "%dx%d_%dx%d" % (s[0] + s[1]))
def test_in_place_behind_a_window_copy(rip_lib, shape):
    """A window of the picture's size without a target: the resize copies it into the caller's buffer, CLAHE runs there in place."""
    import torch
    (w, h), tiles = shape
    k = CC.SHAPES.index(shape)
    p, twin = plain_pipe(), plain_pipe()
    for q in (p, twin):
        q.set_output_roi(3, 2, w, h)
    for i in range(4):
        content, clip, n, layout = CC.CONTENTS[(k + i) % 4], CC.CLIPS[(k + 2 * i) % 5], (3, 1, 5)[(k + i) % 3], CC.LAYOUTS[(k + i + 1) % len(CC.LAYOUTS)]
        t = torch.from_numpy(pictures(content, n, h + 5, w + 7, seed=7 * k + i)).cuda()
        want = expected(twin.apply_device(t, "mono8").cpu().numpy(), (0, 0, w, h), clip, tiles)
        p.set_output_clahe(clip, *tiles)
        deliver_into_layout(p, t, "mono8", want, layout)


# ---- behind the chain ----------------------------------------------------------------------------------------------------------------
MONO_FLIP = "mono_flip_gamma"
CONTEXTS = {
    # (frame, pipeline settings beyond the frame's, head, tiles, clip)
    MONO_FLIP: ("mono65", dict(gamma=True, flip=True, flip_angle=90), HC.Head(), (4, 8), 3.0),
    "mono_flip_gamma_mono8": ("mono65", dict(gamma=True, flip=True, flip_angle=180), HC.Head(format="mono8"), (8, 4), 0.0),
    "bayer_full_chain_undistorted": ("und200", None, HC.Head(format="mono8"), (8, 8), 3.0),
    "bayer_plain": ("bayer136", None, HC.Head(format="mono8"), (8, 8), 40.0),
    "linear": ("bayer136", None, HC.Head(format="mono8", size=(64, 48)), (8, 8), 3.0),
    "area": ("bayer136", None, HC.Head(format="mono8", size=(50, 30), interp="area"), (3, 5), 2.0),
    "linear_aa": ("und200", None, HC.Head(format="mono8", size=(96, 64), interp="linear_aa"), (8, 8), 3.0),
    "window": ("bayer136", None, HC.Head(format="mono8", roi=(8, 4, 64, 32)), (16, 16), 0.01),
    "window_of_a_mono_frame": ("mono65", None, HC.Head(roi=(5, 3, 47, 21)), (4, 2), 3.0),
    "resized_mono_frame": ("mono65", None, HC.Head(size=(40, 20)), (5, 3), 1e9),
    "crop": ("und200", None, HC.Head(format="mono8", size=(96, 64), interp="cubic_aa", fit="crop"), (8, 8), 3.0),
    "letterbox": ("bayer136", None, HC.Head(format="mono8", size=(64, 48), fit="letterbox"), (8, 8), 3.0),
    "letterbox_side_bands": ("bayer136", None, HC.Head(format="mono8", size=(70, 30), fit="letterbox", pad=(3, 128, 250)), (4, 4), 3.0),
}


def context_pipe(name, clahe=True, pad=None):
    frame, settings, head, tiles, clip = CONTEXTS[name]
    p = RawImagePipeline(False, "", "", "", device=0)
    if settings is None:
        HC.configure_pipeline(p, frame)
    else:
        configure(p, cfg(**settings))
    HC.apply_head(p, head if pad is None else head._replace(pad=pad))
    if clahe:
        p.set_output_clahe(clip, *tiles)
    return p


@gpu
@pytest.mark.parametrize("name", sorted(CONTEXTS))
def test_behind_the_chain(rip_lib, name):
    import torch
    frame, _, head, tiles, clip = CONTEXTS[name]
    f = HC.FRAMES[frame]
    twin, p = context_pipe(name, clahe=False), context_pipe(name)
    t = torch.from_numpy(HC.gen_frames(frame, 3, seed=3)).cuda()
    delivered = twin.apply_device(t, f.encoding).cpu().numpy()
    rect = p.get_output_window(f.size[1], f.size[0], 1, f.encoding)[1]
    assert rect == twin.get_output_window(f.size[1], f.size[0], 1, f.encoding)[1]
    p.apply_device(t, f.encoding)          # whatever a handle launches once -- maps, tables -- is behind both
    with twin.launch_log() as off_log:
        twin.apply_device(t, f.encoding)
        torch.cuda.synchronize()
    with p.launch_log() as log:
        got = p.apply_device(t, f.encoding)
        torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == delivered.shape and delivered.ndim == 3
    assert np.array_equal(got.cpu().numpy(), expected(delivered, rect, clip, tiles)), name
    # exactly the two launches behind what the head launched without it
    assert log.names() == off_log.names() + KERNELS
    # strided destinations with sentinels: the in-place paths write the caller's buffer at any alignment
    for layout in CC.LAYOUTS[1:]:
        deliver_into_layout(p, t, f.encoding, expected(delivered, rect, clip, tiles), layout)


@gpu
@pytest.mark.parametrize("name", ["letterbox", "letterbox_side_bands"])
def test_letterbox_bands_hold_the_grey_pad_and_take_no_part(rip_lib, name):
    import torch
    import output_reference
    frame, _, head, tiles, clip = CONTEXTS[name]
    f = HC.FRAMES[frame]
    t = torch.from_numpy(HC.gen_frames(frame, 2, seed=5)).cuda()
    outs = []
    for pad in ((3, 128, 250), (200, 10, 60)):
        p = context_pipe(name, pad=pad)
        x, y, w, h = p.get_output_window(f.size[1], f.size[0], 1, f.encoding)[1]
        assert (w, h) != head.size
        out = p.apply_device(t, f.encoding).cpu().numpy()
        inside = np.zeros(out.shape[1:], bool)
        inside[y:y + h, x:x + w] = True
        grey = int(output_reference.mono8(np.array(pad, np.uint8).reshape(1, 1, 3))[0, 0])
        assert (out[:, ~inside] == grey).all()
        outs.append(out[:, inside])
    assert np.array_equal(outs[0], outs[1])


# ---- heads -----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_three_heads_from_one_run(rip_lib):
    """A colour native head, a plain mono8 head and a mono8 + CLAHE head: each byte for byte what a single-head handle with that
    output delivers; the colour head is still written directly (624 bytes per row of F)."""
    import torch
    frame = "und208"
    f = HC.FRAMES[frame]
    heads = (HC.IDENTITY, HC.Head(format="mono8"), HC.Head(format="mono8", size=(96, 64), fit="letterbox"))
    p = RawImagePipeline(False, "", "", "", device=0)
    HC.configure_pipeline(p, frame)
    HC.configure_heads(p, heads)
    p.select_output_head(2)
    p.set_output_clahe(3.0, 8, 8)
    p.select_output_head(0)
    t = torch.from_numpy(HC.gen_frames(frame, 2, seed=1)).cuda()
    with p.launch_log() as log:
        outs = p.apply_device_heads(t, f.encoding)
        torch.cuda.synchronize()
    assert p.debug_output_head_info(0)[1] == 1 and p.debug_output_head_info(1)[1:] == (0, 0) and p.debug_output_head_info(2)[1:] == (0, 0)
    assert [n for n in log.names() if "clahe" in n] == KERNELS and log.names()[-2:] == KERNELS
    for k, head in enumerate(heads):
        single = RawImagePipeline(False, "", "", "", device=0)
        HC.configure_pipeline(single, frame)
        HC.apply_head(single, head)
        if k == 2:
            single.set_output_clahe(3.0, 8, 8)
        assert torch.equal(outs[k].cpu(), single.apply_device(t, f.encoding).cpu()), k
    # ... and head 2 is the reference on head 2 without CLAHE
    p.select_output_head(2)
    rect = p.get_output_window(f.size[1], f.size[0], 1, f.encoding)[1]
    p.set_output_clahe(0.0, 0, 0)
    plain = p.apply_device_heads(t, f.encoding, heads=[2])[2].cpu().numpy()
    assert np.array_equal(outs[2].cpu().numpy(), expected(plain, rect, 3.0, (8, 8)))


@gpu
def test_a_mono_native_head_with_clahe_is_no_identity_head(rip_lib):
    """Two native heads of a mono camera, one with CLAHE: the plain one is written directly or copied as before, the other goes
    through the staging image and is never the direct head."""
    import torch
    pics = pictures("random", 3, 48, 64, seed=4)          # 64 bytes per row: a tight identity head is written directly
    p = plain_pipe()
    p.set_output_heads(2)
    p.set_output_clahe(3.0, 8, 8)          # head 0
    t = torch.from_numpy(pics).cuda()
    outs = p.apply_device_heads(t, "mono8")
    assert p.debug_output_head_info(0)[1:] == (0, 0) and p.debug_output_head_info(1)[1] == 1
    assert np.array_equal(outs[1].cpu().numpy(), pics)
    assert np.array_equal(outs[0].cpu().numpy(), expected(pics, (0, 0, 64, 48), 3.0, (8, 8)))


# ---- state on one handle ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", [MONO_FLIP, "linear"])
def test_on_other_tiles_off_on_one_handle(rip_lib, name):
    import torch
    frame, _, head, tiles, clip = CONTEXTS[name]
    f = HC.FRAMES[frame]
    t = torch.from_numpy(HC.gen_frames(frame, 2, seed=6)).cuda()
    never = context_pipe(name, clahe=False)
    never.apply_device(t, f.encoding)          # whatever a handle launches once is behind it
    with never.launch_log() as never_log:
        delivered = never.apply_device(t, f.encoding).cpu().numpy()
        torch.cuda.synchronize()
    p = context_pipe(name, clahe=False)
    p.apply_device(t, f.encoding)
    rect = p.get_output_window(f.size[1], f.size[0], 1, f.encoding)[1]
    for clip_k, tiles_k in ((clip, tiles), (clip, (2, 3)), (0.5, (2, 3)), (0.0, (0, 0)), (3.0, (1, 1)), (7.0, (0, 0))):
        p.set_output_clahe(clip_k, *tiles_k)
        with p.launch_log() as log:
            got = p.apply_device(t, f.encoding).cpu().numpy()
            torch.cuda.synchronize()
        if tiles_k == (0, 0):          # off: the launches and the bytes of a handle that never turned it on
            assert log.records() == never_log.records() and np.array_equal(got, delivered)
        else:
            assert log.names() == never_log.names() + KERNELS
            assert np.array_equal(got, expected(delivered, rect, clip_k, tiles_k)), (clip_k, tiles_k)


# ---- ccc, host paths, refusals ------------------------------------------------------------------------------------------------------------
@gpu
def test_ccc_sequence_with_a_refused_frame_in_between(rip_lib):
    pipes = []
    for on in (False, True):
        p = RawImagePipeline(False, "", "", "", device=0)
        p.set_ccc_model(*synth.ccc_model())
        p.set_ccc_kalman_model(1.0, 10.0)
        configure(p, cfg(wb=True, wb_method="ccc", wb_bright=0.8, wb_dark=0.2, wb_temporal=True, gamma=True, gamma_k=0.9))
        p.reset_white_balance_temporal_consistency()
        p.set_output_format("mono8")
        if on:
            p.set_output_clahe(3.0, 8, 8)
        pipes.append(p)
    twin, p = pipes
    frames = [synth.gen_frame(136, 72, BAYER, seed=20 + i) for i in range(4)]
    small = synth.gen_frame(14, 72, BAYER, seed=99)          # 14 columns: fewer than two per tile
    for i, f in enumerate(frames):
        want = twin.process(f, BAYER)
        assert np.array_equal(p.process(f, BAYER), CL.clahe(want, 3.0, 8, 8)), i
        assert np.array_equal(p.get_ccc_track(1), twin.get_ccc_track(1)), i
        if i == 1:          # refused before anything is enqueued: the track is where it was
            before = p.get_ccc_track(1).copy()
            with pytest.raises(ValueError, match="output clahe: the delivered picture of 14 x 72"):
                p.process(small, BAYER)
            assert np.array_equal(p.get_ccc_track(1), before)


@gpu
@pytest.mark.parametrize("name", [MONO_FLIP, "letterbox"])
def test_host_paths(rip_lib, name):
    frame, _, head, tiles, clip = CONTEXTS[name]
    f = HC.FRAMES[frame]
    frames = HC.gen_frames(frame, 3, seed=4)
    twin, p = context_pipe(name, clahe=False), context_pipe(name)
    rect = p.get_output_window(f.size[1], f.size[0], 1, f.encoding)[1]
    wants = [CL.apply_to_delivered(twin.process(x, f.encoding), rect, clip, *tiles) for x in frames]
    got = p.process(frames[0], f.encoding)
    assert got.dtype == np.uint8 and np.array_equal(got, wants[0])
    assert p.get_processed_image().size == 0          # the delivered buffer is the result
    assert np.array_equal(p.apply(frames[1].copy(), f.encoding), wants[1])
    tickets = [p.submit(x, f.encoding) for x in frames]
    for tk, want in zip(tickets, wants):
        assert np.array_equal(p.collect(tk), want)
    assert p.get_processed_image().size == 0
    out = P.host_alloc(wants[2].shape)
    tk = p.submit(frames[2], f.encoding, out=out)
    p.collect(tk)
    assert np.array_equal(out, wants[2])
    p.set_output_heads(2)
    res = p.apply_heads(frames[0], f.encoding)
    assert np.array_equal(res[0], wants[0]) and res[1] is not None and res[1].dtype == np.uint8


@gpu
def test_refusals_of_the_frame_calls(rip_lib):
    import torch
    backing = torch.full((1 << 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    p = plain_pipe()
    p.set_output_clahe(3.0, 8, 8)
    bgr = torch.zeros((1, 32, 48, 3), dtype=torch.uint8, device="cuda")
    for fmt in ("native", "rgb8", "nv12"):
        p.set_output_format(fmt)
        st, msg = raw_apply_device(p, bgr, "bgr8", backing.data_ptr(), 0, 0)
        assert st == P.RIP_ERR_INVALID_ARGUMENT and "output clahe needs a delivered one-channel" in msg and "'mono8'" in msg
    p.set_output_format("mono8")
    st, msg = raw_apply_device(p, bgr, "bgr8", backing.data_ptr(), 0, 0)
    assert st == P.RIP_OK, msg
    for shape in ((1, 15, 48, 3), (1, 32, 15, 3)):
        st, msg = raw_apply_device(p, torch.zeros(shape, dtype=torch.uint8, device="cuda"), "bgr8", backing.data_ptr(), 0, 0)
        assert st == P.RIP_ERR_INVALID_ARGUMENT and "smaller than two pixels per tile" in msg
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="smaller than two pixels per tile"):
        p.process(np.zeros((15, 48, 3), np.uint8), "bgr8")
    with pytest.raises(ValueError, match="smaller than two pixels per tile"):
        p.submit(np.zeros((15, 48, 3), np.uint8), "bgr8")
    p.set_output_heads(2)
    p.select_output_head(1)
    p.set_output_clahe(3.0, 4, 4)
    with pytest.raises(ValueError, match="output head 1: output clahe needs"):
        p.apply_device_heads(bgr, "bgr8")
    with pytest.raises(ValueError, match="output head 1: output clahe needs"):
        p.apply_heads(np.zeros((32, 48, 3), np.uint8), "bgr8")
    assert (backing.cpu().numpy()[32 * 48:] == SENTINEL).all()


# ---- fuzz ---------------------------------------------------------------------------------------------------------------------------------
def test_the_fuzz_draws_what_it_claims():
    cases = [CC.fuzz_case(s) for s in range(CC.FUZZ_CASES)]
    assert len(cases) == 40
    assert {c["frames"] for c in cases} == {1, 3, 5} and {c["content"] for c in cases} == set(CC.CONTENTS) and {c["resized"] for c in cases} == {False, True}
    assert {c["layout"] for c in cases} == set(CC.LAYOUTS) and {c["clip"] for c in cases} >= set(CC.CLIPS)
    assert any(c["width"] % c["tiles"][0] == 0 and c["height"] % c["tiles"][1] for c in cases) and any(c["width"] % c["tiles"][0] for c in cases)
    for c in cases:
        assert c["width"] >= 2 * c["tiles"][0] and c["height"] >= 2 * c["tiles"][1]


@gpu
def test_fuzz(rip_lib):
    """40 seeded configurations: out of place (a mono frame as it is) and in place (behind a window copy), every layout."""
    import torch
    p, twin = plain_pipe(), plain_pipe()
    for seed in range(CC.FUZZ_CASES):
        c = CC.fuzz_case(seed)
        w, h = c["width"], c["height"]
        for q in (p, twin):
            q.set_output_roi(*((2, 1, w, h) if c["resized"] else (0, 0, 0, 0)))
        margin = (4, 3) if c["resized"] else (0, 0)
        t = torch.from_numpy(pictures(c["content"], c["frames"], h + margin[1], w + margin[0], seed=seed)).cuda()
        delivered = twin.apply_device(t, "mono8").cpu().numpy()
        assert delivered.shape == (c["frames"], h, w)
        p.set_output_clahe(c["clip"], *c["tiles"])
        try:
            deliver_into_layout(p, t, "mono8", expected(delivered, (0, 0, w, h), c["clip"], c["tiles"]), c["layout"])
        except AssertionError as e:
            raise AssertionError("configuration %d %r: %s" % (seed, c, e)) from None
