"""Output heads on the GPU (include/rip.h rip_apply_device_heads, rip_apply_heads; PARITY.md "Output heads").  The expectation of every
delivered byte is the single-output path on a twin handle: the same pipeline settings, its only output the head's settings, the same
buffer layout.  Everything at tolerance 0, float formats as bytes; the bytes around the delivered rows hold a sentinel that must
survive in both."""
import ctypes as C

import numpy as np
import pytest

import heads_cases as HC
import heads_variant_cases as HV
from helpers import cfg, configure, device_batch
from raw_image_pipeline_amd import RawImagePipeline, synth
from raw_image_pipeline_amd import pipeline as P

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
LAYOUTS = ("tight", "elem", "p16")
STAGE = ("resize_kernel", "area_reduce_kernel", "fit_", "aa_kernel", "output_convert_kernel", "head_copy_kernel")  # the launches behind F


def gpu_pipe_for(frame, heads=None, head=None):
    p = RawImagePipeline(False, "", "", "", device=0)
    HC.configure_pipeline(p, frame)
    if heads is not None:
        HC.configure_heads(p, heads)
    if head is not None:
        HC.apply_head(p, head)
    return p


class Dest:
    """A head's destination: n delivered frames as a strided region of one flat byte buffer on the device filled with SENTINEL.
    tight: no padding.  elem: the base one element in, rows three elements and frames five elements further apart.  p16: base, pitch
    and frame stride multiples of 16 bytes with padding.  `base_shift` moves the base by that many further bytes."""

    def __init__(self, info, n, layout, base_shift=0):
        import torch
        rows, cols, cn, enc, fmt = info
        dtype, planar, _ = P.OUTPUT_FORMATS.get(enc, (np.uint8, False, cn)) if fmt != "native" else (np.uint8, False, cn)
        e = np.dtype(dtype).itemsize
        row = cols * e if planar else cols * cn * e
        lines = rows * 3 if planar else rows
        off, step, frame = base_shift, row, row * lines
        if layout == "elem":
            off, step = off + e, row + 3 * e
            frame = step * lines + 5 * e
        elif layout == "p16":
            step = (row + 15) // 16 * 16 + 16
            frame = step * lines + 32
        self.total = off + frame * (n - 1) + step * (lines - 1) + row + 8
        self.backing = torch.full((self.total,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.backing.data_ptr() % 16 == 0
        self.off, self.step, self.frame, self.row, self.lines, self.n = off, step, frame, row, lines, n
        self.ptr = self.backing.data_ptr() + off
        self.tight = layout == "tight"

    def head_buffer(self):
        return P._HeadBuffer(C.c_void_p(self.ptr), 0 if self.tight else self.step, 0 if self.tight else self.frame)

    def payload_mask(self):
        m = np.zeros(self.total, bool)
        for f in range(self.n):
            for y in range(self.lines):
                at = self.off + f * self.frame + y * self.step
                m[at:at + self.row] = True
        return m

    def host(self):
        return self.backing.cpu().numpy()


def c_input(frames_t):
    n, rows, cols = frames_t.shape
    return C.c_void_p(frames_t.data_ptr()), C.c_size_t(frames_t.stride(1)), C.c_size_t(frames_t.stride(0) if n > 1 else 0), int(n), int(rows), int(cols)


def tap_tensors(pipe, frames_t, enc):
    import torch
    n, rows, cols = frames_t.shape
    tr, tc, tcn = pipe.query_taps(rows, cols, 1, enc)
    shape = (n, tr, tc) if tcn == 1 else (n, tr, tc, tcn)
    return [torch.full(shape, SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)]


def call_heads(pipe, frames_t, enc, dests, taps=(None, None)):
    """rip_apply_device_heads through the C ABI; dests: one Dest or None per head of the handle.  Returns (status, message)."""
    bufs = (P._HeadBuffer * len(dests))()
    for k, d in enumerate(dests):
        if d is not None:
            bufs[k] = d.head_buffer()
    d_in, in_step, in_frame, n, rows, cols = c_input(frames_t)
    st = pipe._lib.rip_apply_device_heads(pipe._h, d_in, in_step, in_frame, n, rows, cols, 1, enc.encode(), bufs, len(dests),
                                          C.c_void_p(taps[0].data_ptr() if taps[0] is not None else 0), C.c_void_p(taps[1].data_ptr() if taps[1] is not None else 0))
    return st, pipe._lib.rip_last_error(pipe._h).decode()


def call_single(pipe, frames_t, enc, dest, taps=(None, None)):
    d_in, in_step, in_frame, n, rows, cols = c_input(frames_t)
    b = dest.head_buffer()
    st = pipe._lib.rip_apply_device(pipe._h, d_in, in_step, in_frame, n, rows, cols, 1, enc.encode(), C.c_void_p(b.d_out), C.c_size_t(b.out_step),
                                    C.c_size_t(b.out_frame_stride), C.c_void_p(taps[0].data_ptr() if taps[0] is not None else 0),
                                    C.c_void_p(taps[1].data_ptr() if taps[1] is not None else 0))
    return st, pipe._lib.rip_last_error(pipe._h).decode()


def head_infos(pipe, frame, heads):
    """(rows, cols, channels, encoding, format) of the heads `heads` (indices) for a frame of FRAMES[frame]; None elsewhere."""
    f = HC.FRAMES[frame]
    return pipe._head_queries(heads, f.size[1], f.size[0], 1, f.encoding)


def compare_with_twins(frame, heads, frames_t, requested=None, layouts=None, taps=True, pipe=None, shifts=None, what=""):
    """Runs one heads call and, per requested head, the single-output call of a twin into a destination of the same layout; every byte
    of every backing buffer is compared, and the bytes outside the delivered rows must still hold the sentinel.  Returns (pipe, log)."""
    import torch
    enc = HC.FRAMES[frame].encoding
    pipe = pipe or gpu_pipe_for(frame, heads)
    n_heads = len(heads)
    requested = list(range(n_heads)) if requested is None else list(requested)
    infos = head_infos(pipe, frame, requested)
    n = frames_t.shape[0]
    layouts = layouts or [LAYOUTS[k % 3] for k in range(n_heads)]
    shifts = shifts or [0] * n_heads
    dests = [Dest(infos[k], n, layouts[k], shifts[k]) if k in requested else None for k in range(n_heads)]
    my_taps = tap_tensors(pipe, frames_t, enc) if taps else (None, None)
    with pipe.launch_log() as log:
        st, msg = call_heads(pipe, frames_t, enc, dests, my_taps)
        assert st == P.RIP_OK, msg
        torch.cuda.synchronize()
    wb = pipe.get_white_balance_info(n)
    for i, k in enumerate(requested):
        twin = gpu_pipe_for(frame, head=heads[k])
        want = Dest(infos[k], n, layouts[k], shifts[k])
        twin_taps = tap_tensors(twin, frames_t, enc) if taps and i == 0 else (None, None)
        st, msg = call_single(twin, frames_t, enc, want, twin_taps)
        assert st == P.RIP_OK, msg
        torch.cuda.synchronize()
        got, ref = dests[k].host(), want.host()
        mask = want.payload_mask()
        assert (ref[~mask] == SENTINEL).all(), "%s head %d: the twin wrote outside its rows" % (what, k)
        bad = int((got != ref).sum())
        assert bad == 0, "%s head %d (%s, %s): %d of %d bytes differ from the twin's" % (what, k, heads[k].format, layouts[k], bad, got.size)
        if taps and i == 0:
            for a, b, name in zip(my_taps, twin_taps, ("debayered", "colour")):
                assert torch.equal(a, b), "%s: the %s tap differs from the twin's" % (what, name)
            if HC.FRAMES[frame].cfg.get("wb"):          # without white balance no gains are written
                assert np.array_equal(wb, twin.get_white_balance_info(n)), what
    return pipe, log


def device_frames(frame, n, seed=0, layout=None):
    """[n, rows, cols] on the device: contiguous, or -- layout -- a strided view (helpers.device_batch)."""
    import torch
    frames = HC.gen_frames(frame, n, seed)
    if layout is None:
        return torch.from_numpy(frames).cuda()
    return device_batch(frames, layout, np.random.default_rng(seed)).view


def stage_names(log):
    return [n for n in log.names() if n.startswith(STAGE)]


def chain_names(log):
    return [n for n in log.names() if not n.startswith(STAGE)]


# ---- twin comparison -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("head_set", HC.SETS, ids=HC.set_id)
def test_every_head_of_every_set_equals_its_twin(rip_lib, head_set, n):
    """Every set of tests/heads_cases.py, every head requested: destinations tight, element-aligned with the base one element in, and
    16-byte aligned, rotated over the heads; batches of 3 are a strided view with a frame gap.  Taps and gains are the twin's."""
    frames_t = device_frames(head_set.frame, n, seed=3, layout="frame_gap" if n == 3 else None)
    for rot in range(3):
        layouts = [LAYOUTS[(k + rot) % 3] for k in range(len(head_set.heads))]
        compare_with_twins(head_set.frame, head_set.heads, frames_t, layouts=layouts, what="%s rot %d" % (head_set.name, rot))


def test_head_subsets(rip_lib):
    """Only head 2, and heads 0 and 2: what is not requested is neither planned nor run.  A single requested head has the launch log
    of the single-output call on the twin."""
    import torch
    s = HC.BY_NAME["eight"]
    frames_t = device_frames(s.frame, 3, seed=5)
    pipe, log = compare_with_twins(s.frame, s.heads, frames_t, requested=[2], taps=False, what="only head 2")   # taps change the route
    twin = gpu_pipe_for(s.frame, head=s.heads[2])
    with twin.launch_log() as tlog:
        twin.apply_device(frames_t, HC.FRAMES[s.frame].encoding)
        torch.cuda.synchronize()
    assert log.text == tlog.text and log.text
    pipe, log = compare_with_twins(s.frame, s.heads, frames_t, requested=[0, 2], pipe=pipe, what="heads 0 and 2")
    assert len([n for n in stage_names(log) if n.startswith("output_convert")]) == 2   # rgb_chw_f16 and rgb8, nothing of heads 1, 3 ..
    # a head whose settings refuse the frame does not matter while it is not requested
    pipe.select_output_head(5)
    pipe.set_output_interpolation("area")                 # an upscale under area
    compare_with_twins(s.frame, s.heads, frames_t, requested=[0, 2], pipe=pipe, what="heads 0 and 2 beside a refusing head")
    d = [Dest(head_infos(pipe, s.frame, [0])[0], 3, "tight")] + [None] * 4 + [Dest((100, 300, 3, "bgr8", "native"), 3, "tight")] + [None] * 2
    st, msg = call_heads(pipe, frames_t, HC.FRAMES[s.frame].encoding, d)
    assert st == P.RIP_ERR_INVALID_ARGUMENT and msg.startswith("output head 5: "), msg


# ---- direct write and copy -----------------------------------------------------------------------------------------------------
def test_direct_write_and_copy(rip_lib):
    """208 x 136 with a tight identity head: the chain writes it (direct_write = 1) and no head_copy_kernel runs.  The same head with
    the base 4 bytes in, the 200 x 136 frame, and a second identity head each cost exactly one copy launch."""
    copies = lambda log: [n for n in log.names() if n == "head_copy_kernel"]
    heads = (HC.IDENTITY, HC.CROP_CUBIC)
    frames_t = device_frames("und208", 3, seed=7)
    pipe, log = compare_with_twins("und208", heads, frames_t, layouts=["tight", "tight"], what="direct")
    assert pipe.debug_output_head_info(0)[1:] == (1, 0) and pipe.debug_output_head_info(1)[1:] == (0, 0) and not copies(log), log.text
    pipe, log = compare_with_twins("und208", heads, frames_t, layouts=["tight", "tight"], shifts=[4, 0], pipe=pipe, what="base + 4")
    assert pipe.debug_output_head_info(0)[1:] == (0, 1) and len(copies(log)) == 1, log.text
    pipe, log = compare_with_twins("und208", heads, frames_t, layouts=["p16", "tight"], pipe=pipe, what="a padded 16-byte pitch")
    assert pipe.debug_output_head_info(0)[1:] == (1, 0) and not copies(log), log.text
    frames200 = device_frames("und200", 3, seed=7)
    pipe, log = compare_with_twins("und200", heads, frames200, layouts=["tight", "tight"], what="200 x 136")
    assert pipe.debug_output_head_info(0)[1:] == (0, 1) and len(copies(log)) == 1, log.text
    s = HC.BY_NAME["two_identities_direct"]
    pipe, log = compare_with_twins(s.frame, s.heads, frames_t, layouts=["tight", "tight", "tight"], what="two identities")
    assert [pipe.debug_output_head_info(k)[1:] for k in range(3)] == [(1, 0), (0, 1), (0, 0)] and len(copies(log)) == 1, log.text
    # the first identity head does not qualify, the second does: it is the staging image and the first is copied from it
    pipe, log = compare_with_twins(s.frame, s.heads, frames_t, layouts=["elem", "tight", "tight"], pipe=pipe, what="the second qualifies")
    assert [pipe.debug_output_head_info(k)[1:] for k in range(3)] == [(0, 1), (1, 0), (0, 0)] and len(copies(log)) == 1, log.text


@pytest.mark.parametrize("case", HV.CASES, ids=HV.case_id)
def test_every_kernel_of_the_library_runs(rip_lib, case):
    s = HC.BY_NAME[case.head_set]
    pipe, log = compare_with_twins(s.frame, s.heads, device_frames(s.frame, 3, seed=11), layouts=["tight"] * len(s.heads), what=case.name)
    rec = [r for r in log.records() if r["name"] == case.name]
    assert len(rec) == len(case.copied_heads) and all(r["fc"] == case.fc and r["frames"] == 3 and r["block"] == 256 for r in rec), log.text
    w, h = HC.FRAMES[s.frame].f_size
    assert rec[0]["grid"] == ((w * 3 + 4095) // 4096, h)


# ---- the launch log ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head_set", [HC.BY_NAME["eight"], HC.BY_NAME["mean_upscale_aa"], HC.BY_NAME["no_identity"]], ids=HC.set_id)
def test_the_chain_runs_once_and_the_heads_follow_in_index_order(rip_lib, head_set):
    import torch
    frames_t = device_frames(head_set.frame, 3, seed=13)
    enc = HC.FRAMES[head_set.frame].encoding
    pipe, log = compare_with_twins(head_set.frame, head_set.heads, frames_t, layouts=["tight"] * len(head_set.heads), taps=False, what=head_set.name)
    per_head, chains = [], []
    for k, head in enumerate(head_set.heads):
        twin = gpu_pipe_for(head_set.frame, head=head)
        with twin.launch_log() as tlog:
            twin.apply_device(frames_t, enc)
            torch.cuda.synchronize()
        chains.append(chain_names(tlog))
        per_head.append(stage_names(tlog))
    # every chain, statistics, ccc and remap kernel as often as in the single-output call of the twin whose F lies where this call's
    # does -- the directly written head's, else any head's that stages F --, in front of every head's launch
    direct = [k for k in range(len(head_set.heads)) if pipe.debug_output_head_info(k)[1]]
    twin_chain = chains[direct[0]] if direct else chains[[k for k, st in enumerate(per_head) if st][0]]
    names = log.names()
    assert twin_chain and chain_names(log) == twin_chain and names[:len(twin_chain)] == twin_chain, log.text
    expected = []
    for k, head in enumerate(head_set.heads):
        expected += per_head[k] if per_head[k] else ([] if k in direct else ["head_copy_kernel"])
    assert stage_names(log) == expected, log.text


# ---- table caches ----------------------------------------------------------------------------------------------------------------
def test_each_heads_tables_are_built_once(rip_lib):
    import torch
    s = HC.BY_NAME["mean_upscale_aa"]
    frames_t = device_frames(s.frame, 1, seed=17)
    pipe = gpu_pipe_for(s.frame, s.heads)
    infos = head_infos(pipe, s.frame, range(4))
    dests = [Dest(infos[k], 1, "tight") for k in range(4)]
    builds = []
    for _ in range(3):
        assert call_heads(pipe, frames_t, "bayer_rggb8", dests)[0] == P.RIP_OK
        builds.append([pipe.debug_output_head_info(k)[0] for k in range(4)])
    torch.cuda.synchronize()
    # identity: none; bgr_chw_f32 under the 2 x 2 mean: format table + linear tables; native upscale: linear tables; bf16 aa: both
    assert builds[0] == [0, 2, 1, 2] and builds[1] == builds[0] and builds[2] == builds[0]
    pipe.select_output_head(1)
    pipe.set_output_size(40, 30)
    dests[1] = Dest(head_infos(pipe, s.frame, [1])[1], 1, "tight")
    for _ in range(2):
        assert call_heads(pipe, frames_t, "bayer_rggb8", dests)[0] == P.RIP_OK
    torch.cuda.synchronize()
    assert [pipe.debug_output_head_info(k)[0] for k in range(4)] == [0, 3, 1, 2]
    # the single-output call of the selected head uses that head's entry
    pipe.apply_device(frames_t, "bayer_rggb8")
    assert [pipe.debug_output_head_info(k)[0] for k in range(4)] == [0, 3, 1, 2]


# ---- state on one handle ---------------------------------------------------------------------------------------------------------
def test_heads_calls_and_single_output_calls_interleave_on_one_handle(rip_lib):
    import torch
    s = HC.BY_NAME["eight"]
    enc = HC.FRAMES[s.frame].encoding
    frames_t = device_frames(s.frame, 3, seed=19)
    pipe = gpu_pipe_for(s.frame, s.heads)
    twins = {k: gpu_pipe_for(s.frame, head=s.heads[k]) for k in (0, 3, 6)}
    for k in (3, 0, 6, 3):
        compare_with_twins(s.frame, s.heads, frames_t, requested=[1, 2, 4, 6], pipe=pipe, what="heads call before head %d" % k)
        pipe.select_output_head(k)
        got, want = pipe.apply_device(frames_t, enc), twins[k].apply_device(frames_t, enc)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), "single-output call under head %d" % k
        assert pipe.last_encoding == twins[k].last_encoding


# ---- ccc sequence ----------------------------------------------------------------------------------------------------------------
def test_ccc_sequence_advances_once_per_frame_and_a_refused_call_moves_nothing(rip_lib):
    """Eight frames with temporal consistency through a heads handle (two requested heads) and a twin with one output: the same
    track, gains and pixels.  In between, a heads call whose head 1 asks `area` for an upscale is refused naming head 1 before anything
    is enqueued."""
    import torch
    w, h = HC.FRAMES["bayer136"].size
    filt, bias = synth.ccc_model()
    c = cfg(wb=True, wb_method="ccc", wb_bright=0.8, wb_dark=0.2, wb_temporal=True, gamma=True, gamma_k=0.9)
    heads = (HC.IDENTITY, HC.LETTERBOX_F16)
    pipes = []
    for multi in (True, False):
        p = RawImagePipeline(False, "", "", "", device=0)
        p.set_ccc_model(filt, bias)
        p.set_ccc_kalman_model(1.0, 10.0)
        configure(p, c)
        p.reset_white_balance_temporal_consistency()
        if multi:
            HC.configure_heads(p, heads)
        else:
            HC.apply_head(p, heads[1])
        pipes.append(p)
    multi, twin = pipes
    for i in range(8):
        frame = synth.gen_frame(w, h, "bayer_rggb8", seed=4100 + i, kind="scene", tint=(0.70 + 0.04 * i, 1.0, 0.55))
        batch = torch.from_numpy(frame[None]).cuda()
        got = multi.apply_device_heads(batch, "bayer_rggb8")
        want = twin.apply_device(batch, "bayer_rggb8")
        torch.cuda.synchronize()
        assert torch.equal(got[1].view(torch.uint8), want.view(torch.uint8)), "frame %d" % i
        assert np.array_equal(multi.get_ccc_track(1), twin.get_ccc_track(1)), "frame %d" % i
        assert np.array_equal(multi.get_white_balance_info(1), twin.get_white_balance_info(1)), "frame %d" % i
        if i == 3:
            multi.select_output_head(1)
            multi.set_output_size(300, 100)
            multi.select_output_head(0)
            d = [Dest((h, w, 3, "bgr8", "native"), 1, "tight"), Dest((100, 300, 3, "rgb_chw_f16", "rgb_chw_f16"), 1, "tight")]
            with multi.launch_log() as log:
                st, msg = call_heads(multi, batch, "bayer_rggb8", d)
                assert st == P.RIP_ERR_INVALID_ARGUMENT and msg.startswith("output head 1: "), msg
                with pytest.raises(ValueError, match="^output head 1: "):
                    multi.apply_device_heads(batch, "bayer_rggb8")
            assert not log.records(), log.text
            assert all((x.host() == SENTINEL).all() for x in d)
            multi.select_output_head(1)
            multi.set_output_size(*heads[1].size)
            multi.select_output_head(0)


# ---- chain variety ---------------------------------------------------------------------------------------------------------------
VARIETY = {
    "flip_90": ("bayer136", "bayer_rggb8", dict(flip=True, flip_angle=90, gamma=True), {}),
    "mht": ("bayer136", "bayer_rggb8", dict(wb=True, wb_method="grey_world", gamma=True), dict(method="mht")),
    "packed_12": ("bayer136", "bayer_rggb12p", dict(gamma=True), {}),
    "contracted": ("und200", "bayer_rggb8", dict(wb=True, wb_method="grey_world", cc=True, gamma=True, vig=True, undistort=True), dict(fp=1)),
    "uncontracted": ("und200", "bayer_rggb8", dict(wb=True, wb_method="grey_world", cc=True, gamma=True, vig=True, undistort=True), dict(fp=0)),
}


@pytest.mark.parametrize("name", sorted(VARIETY))
def test_behind_other_chains(rip_lib, name):
    """Flip by 90 degrees (F is 72 x 136), MHT, a packed 12-bit frame and both contraction models, each under one head set; the
    undistorted sets of tests/heads_cases.py cover the remap."""
    import torch
    frame, enc, c, extra = VARIETY[name]
    w, h = HC.FRAMES[frame].size
    if c.get("undistort"):
        c = dict(c, cam=synth.camera_model(w, h))
    swap = c.get("flip_angle") == 90
    heads = (HC.IDENTITY, HC.LETTERBOX_F16, HC.Head(format="mono8", roi=(8, 4, 32, 64) if swap else (8, 4, 64, 32)), HC.AA_BF16, HC.IDENTITY)

    def make(hs=None, head=None):
        p = RawImagePipeline(False, "", "", "", device=0)
        configure(p, cfg(**c))
        if "method" in extra:
            p.set_debayer_method(extra["method"])
        if "fp" in extra:
            p.set_fp_contraction(extra["fp"])
        if hs is not None:
            HC.configure_heads(p, hs)
        if head is not None:
            HC.apply_head(p, head)
        return p
    if enc.endswith("12p"):
        rng = np.random.default_rng(23)
        frames_t = torch.from_numpy(rng.integers(0, 256, (3, h, w * 12 // 8), dtype=np.uint8)).cuda()
    else:
        frames_t = torch.from_numpy(np.stack([synth.gen_frame(w, h, enc, seed=23 + i) for i in range(3)])).cuda()
    pipe = make(hs=heads)
    got = pipe.apply_device_heads(frames_t, enc)
    torch.cuda.synchronize()
    for k, head in enumerate(heads):
        want = make(head=head).apply_device(frames_t, enc)
        torch.cuda.synchronize()
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (name, k)
        assert torch.equal(got[k].view(torch.uint8), want.view(torch.uint8)), "%s head %d" % (name, k)


# ---- special results -------------------------------------------------------------------------------------------------------------
def test_a_bgr16_result_takes_one_head(rip_lib):
    import torch
    w, h = 136, 72
    frames = np.random.default_rng(29).integers(0, 65536, (2, h, w), dtype=np.uint16)
    frames_t = torch.from_numpy(frames.view(np.uint8).reshape(2, h, w * 2)).cuda()
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, cfg())
    pipe.set_debayer_16bit(True)
    pipe.set_output_heads(2)
    twin = RawImagePipeline(False, "", "", "", device=0)
    configure(twin, cfg())
    twin.set_debayer_16bit(True)
    got = pipe.apply_device_heads(frames_t, "bayer_rggb16", heads=[1])
    assert got[0] is None and torch.equal(got[1], twin.apply_device(frames_t, "bayer_rggb16"))
    info = (h, w, 6, "bgr16", "native")
    d = [Dest(info, 2, "tight"), Dest(info, 2, "tight")]
    bufs = (P._HeadBuffer * 2)(d[0].head_buffer(), d[1].head_buffer())
    with pipe.launch_log() as log:
        st = pipe._lib.rip_apply_device_heads(pipe._h, C.c_void_p(frames_t.data_ptr()), C.c_size_t(0), C.c_size_t(0), 2, h, w, 1, b"bayer_rggb16", bufs, 2, None, None)
        msg = pipe._lib.rip_last_error(pipe._h).decode()
    assert st == P.RIP_ERR_INVALID_ARGUMENT and "bgr16" in msg and not log.records()
    # the taps rule comes last
    tap = torch.zeros((2, h, w, 3), dtype=torch.uint8, device="cuda")
    bufs = (P._HeadBuffer * 2)(d[0].head_buffer(), P._HeadBuffer())
    st = pipe._lib.rip_apply_device_heads(pipe._h, C.c_void_p(frames_t.data_ptr()), C.c_size_t(0), C.c_size_t(0), 2, h, w, 1, b"bayer_rggb16", bufs, 2,
                                          C.c_void_p(tap.data_ptr()), None)
    assert st == P.RIP_ERR_INVALID_ARGUMENT and "no taps" in pipe._lib.rip_last_error(pipe._h).decode()


def test_the_refusal_order_of_the_heads_call(rip_lib):
    import torch
    s = HC.BY_NAME["no_identity"]
    frames_t = device_frames(s.frame, 1)
    pipe = gpu_pipe_for(s.frame, s.heads)
    infos = head_infos(pipe, s.frame, range(3))
    dests = [Dest(infos[k], 1, "tight") for k in range(3)]
    lib, h = pipe._lib, pipe._h
    bufs = (P._HeadBuffer * 3)(*[d.head_buffer() for d in dests])
    none = (P._HeadBuffer * 3)()
    args = lambda d_in=frames_t.data_ptr(), b=bufs, enc=b"bayer_rggb8", n=3, rows=72, frames=1: (
        h, C.c_void_p(d_in), C.c_size_t(0), C.c_size_t(0), frames, rows, 136, 1, enc, b, n, None, None)
    msg = lambda: lib.rip_last_error(h).decode()
    assert lib.rip_apply_device_heads(*args(d_in=0, n=2, b=none)) == P.RIP_ERR_INVALID_ARGUMENT and "null" in msg()          # 1 before 2 and 3
    assert lib.rip_apply_device_heads(*args(n=2, b=none)) == P.RIP_ERR_INVALID_ARGUMENT and "3 output heads" in msg()        # 2 before 3
    assert lib.rip_apply_device_heads(*args(b=none, rows=2)) == P.RIP_ERR_INVALID_ARGUMENT and "no head is requested" in msg()  # 3 before 4
    assert lib.rip_apply_device_heads(*args(b=none, frames=0)) == P.RIP_ERR_INVALID_ARGUMENT
    assert lib.rip_apply_device_heads(*args(frames=0)) == P.RIP_OK
    pipe.select_output_head(1)
    pipe.set_output_roi(100, 0, 64, 32)                                                                                        # outside F
    assert lib.rip_apply_device_heads(*args(rows=2)) == P.RIP_ERR_ASSERT                                                       # 4 before 5
    bad0 = (P._HeadBuffer * 3)(P._HeadBuffer(C.c_void_p(dests[0].ptr), 1, 0), dests[1].head_buffer(), dests[2].head_buffer())
    assert lib.rip_apply_device_heads(*args(b=bad0)) == P.RIP_ERR_INVALID_ARGUMENT and msg().startswith("output head 0: output row pitch")   # index order
    assert lib.rip_apply_device_heads(*args()) == P.RIP_ERR_INVALID_ARGUMENT and msg().startswith("output head 1: ") and "does not lie inside" in msg()
    torch.cuda.synchronize()
    assert all((d.host() == SENTINEL).all() for d in dests)


# ---- host path -------------------------------------------------------------------------------------------------------------------
def test_host_path(rip_lib):
    """rip_apply_heads against rip_apply on the twins: bytes, geometry arrays, the capacity refusal, the taps kept and no processed
    image."""
    s = HC.BY_NAME["eight"]
    f = HC.FRAMES[s.frame]
    frame = HC.gen_frames(s.frame, 1, seed=31)[0]
    pipe = gpu_pipe_for(s.frame, s.heads)
    got = pipe.apply_heads(frame, f.encoding)
    twins = [gpu_pipe_for(s.frame, head=h) for h in s.heads]
    for k, t in enumerate(twins):
        want = t.process(frame, f.encoding)
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, k
        assert np.array_equal(got[k].view(np.uint8), want.view(np.uint8)), "head %d" % k
    assert pipe.get_processed_image().size == 0
    for getter in ("get_dist_debayered_image", "get_dist_color_image"):
        assert np.array_equal(getattr(pipe, getter)(), getattr(twins[1], getter)()), getter
    sub = pipe.apply_heads(frame, f.encoding, heads=[6, 1])
    assert [x is not None for x in sub] == [False, True, False, False, False, False, True, False]
    assert np.array_equal(sub[6].view(np.uint8), got[6].view(np.uint8)) and np.array_equal(sub[1], got[1])
    # the geometry arrays and the capacity refusal, through the C ABI
    n = 8
    outs, caps = (C.c_void_p * n)(), (C.c_size_t * n)()
    keep = {k: np.full(got[k].nbytes, SENTINEL, np.uint8) for k in (0, 2)}
    for k, a in keep.items():
        outs[k], caps[k] = a.ctypes.data, a.nbytes
    r, c, ch = (C.c_int * n)(*[-1] * n), (C.c_int * n)(*[-1] * n), (C.c_int * n)(*[-1] * n)
    fr = np.ascontiguousarray(frame)
    call = lambda: pipe._lib.rip_apply_heads(pipe._h, fr.ctypes.data_as(C.c_void_p), f.size[1], f.size[0], 1, C.c_size_t(0), f.encoding.encode(), outs, caps, n, r, c, ch)
    assert call() == P.RIP_OK
    assert (r[0], c[0], ch[0]) == (48, 64, 3) and (r[2], c[2], ch[2]) == (64, 96, 3) and (r[1], c[1], ch[1]) == (0, 0, 0)
    assert np.array_equal(keep[0], got[0].view(np.uint8).ravel()) and np.array_equal(keep[2], got[2].ravel())
    caps[2] -= 1
    keep[0][...] = SENTINEL
    with pipe.launch_log() as log:
        assert call() == P.RIP_ERR_CAPACITY
        assert pipe._lib.rip_last_error(pipe._h).decode().startswith("output head 2: output buffer too small")
    assert not log.records()
    assert (keep[0] == SENTINEL).all()


def test_the_ring_delivers_the_head_selected_at_submit_time(rip_lib):
    """rip_submit keeps the selected head in the slot's plan: selecting another head before rip_collect changes nothing for the frame
    in flight, and rip_set_output_heads is refused while it is."""
    s = HC.BY_NAME["no_identity"]
    f = HC.FRAMES[s.frame]
    frame = HC.gen_frames(s.frame, 1, seed=33)[0]
    pipe = gpu_pipe_for(s.frame, s.heads)
    pipe.select_output_head(1)
    ticket = pipe.submit(frame, f.encoding)
    pipe.select_output_head(2)
    with pytest.raises(ValueError, match="in flight"):
        pipe.set_output_heads(2)
    got = pipe.collect(ticket)
    assert pipe.get_output_heads() == 3 and pipe.get_selected_output_head() == 2
    want = gpu_pipe_for(s.frame, head=s.heads[1]).process(frame, f.encoding)
    assert got.shape == want.shape and np.array_equal(got, want) and pipe.last_encoding == "rgb8"
    assert np.array_equal(pipe.process(frame, f.encoding), gpu_pipe_for(s.frame, head=s.heads[2]).process(frame, f.encoding))
    pipe.set_output_heads(2)


# ---- Python ----------------------------------------------------------------------------------------------------------------------
def test_apply_device_heads_dtypes_and_shapes(rip_lib):
    import torch
    s = HC.BY_NAME["eight"]
    frames_t = device_frames(s.frame, 2, seed=37)
    pipe = gpu_pipe_for(s.frame, s.heads)
    got = pipe.apply_device_heads(frames_t, HC.FRAMES[s.frame].encoding)
    want = [(torch.float16, (2, 3, 48, 64)), (torch.uint8, (2, 136, 208, 3)), (torch.uint8, (2, 64, 96, 3)), (torch.uint8, (2, 32, 64)),
            (torch.float32, (2, 3, 68, 104)), (torch.uint8, (2, 100, 300, 3)), (torch.bfloat16, (2, 3, 40, 50)), (torch.uint8, (2, 136, 208, 3))]
    assert [(t.dtype, tuple(t.shape)) for t in got] == want
    assert torch.equal(got[1], got[7]) and pipe.get_selected_output_head() == 0
    sub = pipe.apply_device_heads(frames_t, HC.FRAMES[s.frame].encoding, heads=[4])
    assert [t is not None for t in sub] == [k == 4 for k in range(8)] and torch.equal(sub[4], got[4])
    # given tensors are written in place; a wrong one is refused
    outs = [None] * 8
    outs[3] = torch.zeros((2, 32, 64), dtype=torch.uint8, device="cuda")
    again = pipe.apply_device_heads(frames_t, HC.FRAMES[s.frame].encoding, heads=[3], outs=outs)
    assert again[3] is outs[3] and torch.equal(outs[3], got[3])
    outs[3] = torch.zeros((2, 32, 65), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match=r"outs\[3\]"):
        pipe.apply_device_heads(frames_t, HC.FRAMES[s.frame].encoding, heads=[3], outs=outs)


# ---- a seeded fuzz -----------------------------------------------------------------------------------------------------------------
FUZZ_CASES = 30
FUZZ_FRAMES = ("bayer136", "und200", "und208", "mono65")


def fuzz_case(seed):
    """2 to 8 heads drawn from the settings the single-output fuzzes draw (format, target, interpolation, window inside F, fit, pad,
    normalisation), a random subset requested, a layout per head.  A head whose draw the filter's own rules refuse (an upscale under
    area, a factor beyond 64 under an antialiased filter) is redrawn as linear."""
    rng = np.random.default_rng(91000 + seed)
    frame = FUZZ_FRAMES[int(rng.integers(len(FUZZ_FRAMES)))]
    f = HC.FRAMES[frame]
    C_, R_ = f.f_size
    mono = f.encoding == "mono8"
    formats = ("native", "mono8") if mono else ("native", "native") + tuple(P.OUTPUT_FORMATS)
    probe = RawImagePipeline(False, "", "", "", device=-1)
    HC.configure_pipeline(probe, frame)
    heads = []
    for _ in range(int(rng.integers(2, 9))):
        roi = (0, 0, 0, 0)
        if rng.random() < 0.5:
            w, h = int(rng.integers(1, C_ + 1)), int(rng.integers(1, R_ + 1))
            roi = (int(rng.integers(0, C_ - w + 1)), int(rng.integers(0, R_ - h + 1)), w, h)
        size = (0, 0)
        if rng.random() < 0.7:
            size = tuple(int(v) for v in rng.integers(1, 260, 2))
        if rng.random() < 0.25:
            roi, size = (0, 0, 0, 0), (0, 0)                                # an identity head under "native"
        head = HC.Head(format=formats[int(rng.integers(len(formats)))], norm=(float(rng.choice([255.0, 1.0, 57.0])), tuple(rng.random(3)), tuple(0.2 + rng.random(3))),
                       size=size, interp=("linear", "area", "linear_aa", "cubic_aa")[int(rng.integers(4))], roi=roi,
                       fit=("stretch", "letterbox", "crop")[int(rng.integers(3))], pad=tuple(int(v) for v in rng.integers(0, 256, 3)))
        HC.apply_head(probe, head)
        try:
            probe.query_output(R_, C_, 1, f.encoding)
        except ValueError:
            head = head._replace(interp="linear")
        heads.append(head)
    requested = [k for k in range(len(heads)) if rng.random() < 0.7] or [int(rng.integers(len(heads)))]
    layouts = [LAYOUTS[int(rng.integers(3))] for _ in heads]
    return frame, tuple(heads), requested, layouts, int(rng.integers(1, 4))


@pytest.mark.parametrize("seed", range(FUZZ_CASES))
def test_fuzz(rip_lib, seed):
    frame, heads, requested, layouts, n = fuzz_case(seed)
    compare_with_twins(frame, heads, device_frames(frame, n, seed=seed), requested=requested, layouts=layouts, what="fuzz %d" % seed)


def test_the_fuzz_draws_what_it_claims():
    cases = [fuzz_case(s) for s in range(FUZZ_CASES)]
    assert {c[0] for c in cases} == set(FUZZ_FRAMES)
    assert {len(c[1]) for c in cases} >= {2, 8} and any(len(c[2]) < len(c[1]) for c in cases) and any(len(c[2]) == 1 for c in cases)
    heads = [h for c in cases for k, h in enumerate(c[1]) if k in c[2]]
    assert {h.interp for h in heads} == {"linear", "area", "linear_aa", "cubic_aa"} and {h.fit for h in heads} == {"stretch", "letterbox", "crop"}
    assert {h.format for h in heads} >= set(P.OUTPUT_FORMATS) | {"native"}
    assert sum(h.format == "native" and h.size == (0, 0) and h.roi == (0, 0, 0, 0) for h in heads) >= 5
