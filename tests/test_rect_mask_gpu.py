"""Valid-pixel masks on the GPU (include/rip.h rip_set_rect_mask, rip_get_output_mask; PARITY.md "Rect mask").  Two expectations pin
everything, both at tolerance 0: the coverage M is the oracle's remap of an all-255 image through the handle's own maps, and a head's
delivered mask M' is what a twin handle with every stage off delivers for M as a mono8 frame under that head's window, size, fit and
interpolation, format native, pad (0, 0, 0); `valid` is the threshold of either."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import heads_cases as HC
import mask_cases as MC
import mask_variant_cases as MV
from helpers import cfg, configure
from raw_image_pipeline_amd import RawImagePipeline, synth
from raw_image_pipeline_amd import pipeline as P
from test_cpp_facade import BRANCHES, run_env
from test_rect_mask import build_facade_program

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
MASK_KERNELS = ("rect_mask_kernel<false>", "rect_mask_kernel<true>", "mask_threshold_kernel")


def und_pipe(size, pair=(0.0, 1.0), model="equidistant", cam=None, flip=None, mode="coverage"):
    """Undistortion only: what a mono8 frame needs to come out as its remap."""
    p = RawImagePipeline(False, "", "", "", device=0)
    c = cfg(undistort=True, cam=cam or synth.camera_model(*size), balance=pair[0], fov_scale=pair[1])
    if flip:
        c.update(flip=True, flip_angle=flip)
    if model != "equidistant":
        c["cam"] = None
    configure(p, c)
    if model != "equidistant":
        synth.load_camera(p, cam, model)
        p.set_undistortion_balance(pair[0])
        p.set_undistortion_fov_scale(pair[1])
    p.set_rect_mask(mode)
    return p


def oracle_mask(O, pipe, src_size):
    mx, my = pipe.get_undistortion_maps()
    return MC.expected(O, mx, my, src_size)


def twin_delivers(m, head):
    """What the single-output path delivers for the one-channel image m under `head`'s geometry, format native, pad (0, 0, 0)."""
    import torch
    t = RawImagePipeline(False, "", "", "", device=0)
    configure(t, cfg())
    HC.apply_head(t, HC.Head(size=head.size, interp=head.interp, roi=head.roi, fit=head.fit, pad=(0, 0, 0)))
    out = t.apply_device(torch.from_numpy(np.ascontiguousarray(m)[None]).cuda(), "mono8")
    torch.cuda.synchronize()
    return out[0].cpu().numpy()


def read_device(ptr, pitch, h, w):
    """h x w bytes at a raw device pointer, rows `pitch` bytes apart."""
    import torch
    torch.cuda.synchronize()
    hip = C.CDLL("libamdhip64.so")          # the runtime torch has loaded
    hip.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    out = np.empty((h, w), np.uint8)
    assert hip.hipMemcpy2D(out.ctypes.data_as(C.c_void_p), w, C.c_void_p(ptr), pitch, w, h, 2) == 0
    return out


def frame_of(size, value=255):
    return np.full((size[1], size[0]), value, np.uint8)


# ---- against the oracle, and against the pipeline itself --------------------------------------------------------------------------
@pytest.mark.parametrize("size", MC.SIZES, ids=lambda s: "%dx%d" % s)
def test_rect_mask_equals_the_oracles_remap_of_white(oracle, size):
    for pair in MC.PAIRS:
        p = und_pipe(size, pair)
        white = p.process(frame_of(size), "mono8")
        want = oracle_mask(oracle, p, size)
        MC.assert_classes(want, pair, "%s %s" % (size, pair))
        got = p.get_rect_mask()
        assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want), (size, pair, int((got != want).sum()))
        assert np.array_equal(got, white), "the mask differs from the undistorted all-255 frame"          # against the pipeline itself
        p.set_rect_mask("valid")
        assert np.array_equal(p.get_rect_mask(), MC.valid_of(want)), (size, pair)
        # the view: geometry with a null pointer, the mask lives on the device
        view, r, c, k = C.c_void_p(1), C.c_int(), C.c_int(), C.c_int()
        assert p._lib.rip_get_image_view(p._h, P.IMAGE_RECT_MASK, C.byref(view), C.byref(r), C.byref(c), C.byref(k)) == P.RIP_OK
        assert (view.value, r.value, c.value, k.value) == (None, size[1], size[0], 1)
        p.set_rect_mask("off")
        assert p.get_rect_mask().shape == (0, 0)


def test_plumb_bob_with_balance_one(oracle):
    size = (200, 136)
    cam = synth.pinhole_camera_model(*size, (-0.28, 0.07, 0.0005, -0.0003, 0.0))
    p = und_pipe(size, (1.0, 1.0), model="plumb_bob", cam=cam)
    white = p.process(frame_of(size), "mono8")
    want = oracle_mask(oracle, p, size)
    z, part, full = MC.classes(want)
    assert z > 0 and part > 0 and full > 0
    assert np.array_equal(p.get_rect_mask(), want) and np.array_equal(white, want)
    p.set_rect_mask("valid")
    assert np.array_equal(p.get_rect_mask(), MC.valid_of(want))


# (width, rows): the fov_scale under balance 1 at which the expectation holds at least two distinct values (asserted below)
NARROW = {(3, 3): 1.0, (4, 4): 2.5, (5, 5): 2.5, (7, 3): 1.6, (1023, 4): 1.6, (1025, 5): 1.6}


@pytest.mark.parametrize("size", sorted(NARROW), ids=lambda s: "%dx%d" % s)
def test_narrow_and_edge_widths(oracle, size):
    p = und_pipe(size, (1.0, NARROW[size]))
    white = p.process(frame_of(size), "mono8")
    want = oracle_mask(oracle, p, size)
    assert len(np.unique(want)) >= 2, "fov_scale %s gives a constant mask at %s" % (NARROW[size], size)
    assert np.array_equal(p.get_rect_mask(), want) and np.array_equal(white, want), size
    p.set_rect_mask("valid")
    assert np.array_equal(p.get_rect_mask(), MC.valid_of(want))
    assert np.array_equal(p.get_output_mask(size[1], size[0], 1, "mono8"), MC.valid_of(want))


def test_a_smaller_source_and_flip_90(oracle):
    # a 136 x 72 frame under a 200 x 136 calibration: the maps keep their size, the taps beyond the source are border
    p = und_pipe((200, 136), (1.0, 1.0))
    white = p.process(frame_of((136, 72)), "mono8")
    want = oracle_mask(oracle, p, (136, 72))
    assert want.shape == (136, 200) and all(v > 0 for v in MC.classes(want))
    assert np.array_equal(p.get_rect_mask(), want) and np.array_equal(white, want)
    # the same handle, a frame of the calibration's size: M is rebuilt for the new source size
    white = p.process(frame_of((200, 136)), "mono8")
    full = oracle_mask(oracle, p, (200, 136))
    assert not np.array_equal(full, want) and np.array_equal(p.get_rect_mask(), full) and np.array_equal(white, full)
    # flip 90: the image that enters the remap is 136 wide and 200 high
    p = und_pipe((200, 136), (1.0, 1.0), flip=90)
    white = p.process(frame_of((200, 136)), "mono8")
    want = oracle_mask(oracle, p, (136, 200))
    assert all(v > 0 for v in MC.classes(want)) and not np.array_equal(want, full)
    assert np.array_equal(p.get_rect_mask(), want) and np.array_equal(white, want)
    assert np.array_equal(p.get_output_mask(136, 200, 1, "mono8"), want)


# ---- heads ----------------------------------------------------------------------------------------------------------------------
def base_mask(O, probe, frame):
    """M of a FRAMES entry: the coverage of its undistortion, or all 255 at F's size."""
    f = HC.FRAMES[frame]
    if f.cfg.get("undistort"):
        return oracle_mask(O, probe, f.size)
    return frame_of(f.f_size)


@pytest.mark.parametrize("head_set", HC.SETS, ids=HC.set_id)
def test_every_head_of_every_set_equals_the_twin_fed_the_mask(oracle, head_set):
    f = HC.FRAMES[head_set.frame]
    p = RawImagePipeline(False, "", "", "", device=0)
    HC.configure_pipeline(p, head_set.frame)
    HC.configure_heads(p, head_set.heads)
    geometry = (f.size[1], f.size[0], f.channels, f.encoding)
    m = base_mask(oracle, p, head_set.frame)
    wants = {}
    for mode in ("coverage", "valid"):
        p.set_rect_mask(mode)
        for k, head in enumerate(head_set.heads):
            key = (head.size, head.interp, head.roi, head.fit)
            if key not in wants:
                wants[key] = twin_delivers(m, head)
            want = wants[key] if mode == "coverage" else MC.valid_of(wants[key])
            p.select_output_head(k)
            rows, cols = p.query_output(*geometry)[:2]
            assert want.shape == (rows, cols), (k, want.shape)
            # the host getter, with a sentinel behind H * W
            buf = np.full(rows * cols + 16, SENTINEL, np.uint8)
            h, w = C.c_int(), C.c_int()
            st = p._lib.rip_get_output_mask(p._h, *geometry[:3], geometry[3].encode(), buf.ctypes.data_as(C.c_void_p), C.c_size_t(rows * cols), C.byref(h), C.byref(w))
            assert st == P.RIP_OK and (h.value, w.value) == (rows, cols), p._lib.rip_last_error(p._h).decode()
            got = buf[:rows * cols].reshape(rows, cols)
            assert np.array_equal(got, want), "%s head %d under %s: %d of %d bytes differ" % (head_set.name, k, mode, int((got != want).sum()), got.size)
            assert (buf[rows * cols:] == SENTINEL).all()
            # the device getter's image is the host one
            ptr, pitch, dh, dw = p.get_output_mask_device(*geometry)
            assert (dh, dw) == (rows, cols) and pitch % 16 == 0 and pitch >= cols and ptr % 16 == 0
            assert np.array_equal(read_device(ptr, pitch, rows, cols), want), (head_set.name, k, mode)
            assert np.array_equal(p.get_output_mask(*geometry), want)


def test_frames_that_are_not_undistorted(rip_lib):
    p = RawImagePipeline(False, "", "", "", device=0)
    HC.configure_pipeline(p, "bayer136")
    HC.configure_heads(p, (HC.IDENTITY, HC.LETTERBOX_F16))
    p.set_rect_mask("coverage")
    geometry = (72, 136, 1, "bayer_rggb8")
    with p.launch_log() as log:
        ident = p.get_output_mask(*geometry)
    assert ident.shape == (72, 136) and (ident == 255).all()
    assert not [n for n in log.names() if n in MASK_KERNELS], log.text            # an all-255 image is a fill
    p.select_output_head(1)
    src, dst = p.get_output_window(*geometry)
    box = p.get_output_mask(*geometry)
    assert box.shape == (48, 64) and dst == (0, 7, 64, 34)
    inside = np.zeros_like(box, bool)
    inside[dst[1]:dst[1] + dst[3], dst[0]:dst[0] + dst[2]] = True
    assert (box[inside] == 255).all() and (box[~inside] == 0).all() and (~inside).any()
    p.set_rect_mask("valid")
    assert np.array_equal(p.get_output_mask(*geometry), box)
    # a frame call that was not undistorted leaves the rect mask empty
    p.process(HC.gen_frames("bayer136", 1)[0], "bayer_rggb8")
    assert p.get_rect_mask().shape == (0, 0)


# ---- no effect on frames ---------------------------------------------------------------------------------------------------------
def test_the_mode_changes_nothing_of_a_frame_call(rip_lib):
    """One full-chain configuration with undistortion, three frames, taps on: results, taps and the launch record of the single-output
    call and of a three-head call -- with the head the chain writes directly -- are the same under off, coverage and valid."""
    import torch
    w, h = 208, 136
    heads = (HC.IDENTITY, HC.CROP_CUBIC, HC.LETTERBOX_F16)
    frames_t = torch.from_numpy(np.stack([synth.gen_frame(w, h, "bayer_rggb8", seed=70 + i) for i in range(3)])).cuda()
    seen = {}
    for mode in ("off", "coverage", "valid"):
        p = RawImagePipeline(False, "", "", "", device=0)
        synth.configure_full_chain(p, w, h, "grey_world")
        HC.configure_heads(p, heads)
        p.set_rect_mask(mode)
        taps = [torch.zeros((3, h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(4)]
        with p.launch_log() as log:
            single = p.apply_device(frames_t, "bayer_rggb8", tap_debayered=taps[0], tap_color=taps[1])
            multi = p.apply_device_heads(frames_t, "bayer_rggb8", tap_debayered=taps[2], tap_color=taps[3])
            torch.cuda.synchronize()
        assert p.debug_output_head_info(0)[1] == 1          # the identity head was written by the chain
        assert not [n for n in log.names() if n in MASK_KERNELS] and p.debug_rect_mask_info(0) == (0, 0)
        seen[mode] = (log.text, [t.cpu().numpy() for t in [single] + taps], [t.view(torch.uint8).cpu().numpy() for t in multi])
    for mode in ("coverage", "valid"):
        assert seen[mode][0] == seen["off"][0] and seen["off"][0], mode
        for a, b in zip(seen[mode][1] + seen[mode][2], seen["off"][1] + seen["off"][2]):
            assert np.array_equal(a, b), mode


# ---- cache ---------------------------------------------------------------------------------------------------------------------
def mask_launches(log):
    return [n for n in log.names() if n in MASK_KERNELS]


def test_the_caches(oracle):
    size = (200, 136)
    p = und_pipe(size, (1.0, 1.0))
    HC.configure_heads(p, (HC.IDENTITY, HC.UPSCALE, HC.Head(size=(50, 40), interp="linear_aa")))
    geometry = (size[1], size[0], 1, "mono8")
    with p.launch_log() as log:
        first = p.get_output_mask(*geometry)
    assert mask_launches(log) == ["rect_mask_kernel<false>"] and p.debug_rect_mask_info(0) == (1, 1)
    rec = [r for r in log.records() if r["name"] == "rect_mask_kernel<false>"][0]
    assert rec["grid"] == (1, 136) and rec["block"] == 256 and rec["frames"] == 0
    with p.launch_log() as log:
        assert np.array_equal(p.get_output_mask(*geometry), first)
        p.get_output_mask_device(*geometry)
    assert not log.records() and p.debug_rect_mask_info(0) == (1, 1)             # nothing launched, nothing built
    # head 1: its own resize behind the cached M
    p.select_output_head(1)
    with p.launch_log() as log:
        up = p.get_output_mask(*geometry)
    assert not mask_launches(log) and log.records() and p.debug_rect_mask_info(1) == (1, 1)
    # an output setter on head 1 rebuilds head 1's M' and neither M nor head 0's
    p.set_output_size(150, 90)
    with p.launch_log() as log:
        assert p.get_output_mask(*geometry).shape == (90, 150)
    assert not mask_launches(log) and p.debug_rect_mask_info(1) == (1, 2) and p.debug_rect_mask_info(0) == (1, 1)
    p.set_output_size(150, 90)                                                   # the same value again: still an output setter
    p.get_output_mask(*geometry)
    assert p.debug_rect_mask_info(1) == (1, 3)
    p.select_output_head(0)
    with p.launch_log() as log:
        assert np.array_equal(p.get_output_mask(*geometry), first)
    assert not log.records() and p.debug_rect_mask_info(0) == (1, 1)
    # the balance rebuilds M (and with it every head's M')
    p.set_undistortion_balance(0.5)
    with p.launch_log() as log:
        other = p.get_output_mask(*geometry)
    assert mask_launches(log) == ["rect_mask_kernel<false>"] and p.debug_rect_mask_info(0) == (2, 2)
    assert np.array_equal(other, oracle_mask(oracle, p, size)) and not np.array_equal(other, first)
    # a frame of another size: M is rebuilt for that source
    with p.launch_log() as log:
        small = p.get_output_mask(72, 136, 1, "mono8")
    assert mask_launches(log) == ["rect_mask_kernel<false>"] and p.debug_rect_mask_info(0) == (3, 3)
    assert np.array_equal(small, oracle_mask(oracle, p, (136, 72)))
    # shrinking drops the reset heads' caches
    p.select_output_head(2)
    aa = p.get_output_mask(*geometry)
    assert aa.shape == (40, 50) and p.debug_rect_mask_info(2)[1] == 1
    p.set_output_heads(2)
    p.set_output_heads(3)
    p.select_output_head(2)
    again = p.get_output_mask(*geometry)
    assert again.shape == (136, 200) and p.debug_rect_mask_info(2)[1] == 2       # the defaults now: the identity
    # the mode is part of a head's key: valid is rebuilt, the thresholded twin is one more launch
    p.set_rect_mask("valid")
    with p.launch_log() as log:
        assert np.array_equal(p.get_output_mask(*geometry), MC.valid_of(again))
    assert mask_launches(log) == ["rect_mask_kernel<true>"]
    assert up.shape == (100, 300)


@pytest.mark.parametrize("case", MV.CASES, ids=MV.case_id)
def test_every_kernel_of_the_library_runs(oracle, case):
    f = HC.FRAMES[MV.FRAME]
    p = RawImagePipeline(False, "", "", "", device=0)
    HC.configure_pipeline(p, MV.FRAME)
    HC.apply_head(p, case.head)
    p.set_rect_mask(case.mode)
    with p.launch_log() as log:
        got = p.get_output_mask(f.size[1], f.size[0], f.channels, f.encoding)
    rec = [r for r in log.records() if r["name"] == case.name]
    assert len(rec) == 1 and rec[0]["fc"] == case.fc and rec[0]["block"] == 256, log.text
    want = twin_delivers(oracle_mask(oracle, p, f.size), case.head)
    assert np.array_equal(got, MC.valid_of(want) if case.mode == "valid" else want)


# ---- host paths -------------------------------------------------------------------------------------------------------------------
def test_host_paths(oracle):
    size = (200, 136)
    p = und_pipe(size, (1.0, 1.0))
    want = oracle_mask(oracle, p, size)
    frame = synth.gen_scene_bgr(size[0], size[1], 3)[..., 1].copy()
    # rip_apply, then the getter: the C ABI with its capacity check
    out = p.process(frame, "mono8")
    assert out.shape == (136, 200)
    r, c, k = C.c_int(), C.c_int(), C.c_int()
    buf = np.full(want.size + 8, SENTINEL, np.uint8)
    get = lambda cap: p._lib.rip_get_image(p._h, P.IMAGE_RECT_MASK, buf.ctypes.data_as(C.c_void_p), C.c_size_t(cap), C.byref(r), C.byref(c), C.byref(k))
    assert get(want.size - 1) == P.RIP_ERR_CAPACITY and (buf == SENTINEL).all()
    assert get(want.size) == P.RIP_OK and (r.value, c.value, k.value) == (136, 200, 1)
    assert np.array_equal(buf[:want.size].reshape(want.shape), want) and (buf[want.size:] == SENTINEL).all()
    # submit, collect, then the getter; a frame that is not undistorted in between empties it
    p.set_undistortion(False)
    p.process(frame, "mono8")
    assert p.get_rect_mask().shape == (0, 0)
    p.set_undistortion(True)
    ticket = p.submit(frame, "mono8")
    assert p.get_rect_mask().shape == (0, 0)          # the mask belongs to collected frames
    p.collect(ticket)
    got = p.get_rect_mask()
    assert got.shape == (136, 200) and got.dtype == np.uint8 and np.array_equal(got, want)
    # the heads calls are frame calls too
    p.set_undistortion(False)
    p.apply_heads(frame, "mono8")
    assert p.get_rect_mask().shape == (0, 0)
    p.set_undistortion(True)
    p.apply_heads(frame, "mono8")
    assert np.array_equal(p.get_rect_mask(), want)
    # the Python shapes
    m = p.get_output_mask(136, 200, 1, "mono8")
    assert m.shape == (136, 200) and m.dtype == np.uint8 and m.flags.c_contiguous
    ptr, pitch, h, w = p.get_output_mask_device(136, 200, 1, "mono8")
    assert isinstance(ptr, int) and ptr and (pitch, h, w) == (208, 136, 200)


def test_the_front_end_publishes_the_mask_of_the_delivered_image(oracle, tmp_path):
    from raw_image_pipeline_amd.frontend import CameraStream
    size = (200, 136)
    calib = tmp_path / "calib.yaml"
    calib.write_text(synth.calibration_yaml(synth.camera_model(*size)))
    params = {"input_type": "mono", "undistortion/enabled": True, "undistortion/balance": 1.0, "undistortion/calibration_file": str(calib),
              "rect_mask": "valid", "output_prefix": "/cam0"}
    cam = CameraStream(params, device=0)
    assert "/cam0/image_mask" in cam.topics()
    frame = synth.gen_scene_bgr(size[0], size[1], 5)[..., 1].copy()
    msgs = cam.on_image(frame, "mono8", stamp=1.5)
    topics = [m["topic"] for m in msgs]
    assert topics[:3] == ["/cam0/mono_rect/image", "/cam0/mono_rect/image/slow", "/cam0/image_mask"] and topics.count("/cam0/image_mask") == 1
    mask, rect = msgs[2], msgs[0]
    assert mask["encoding"] == "mono8" and mask["camera_info"] == rect["camera_info"] and mask["header"]["stamp"] == 1.5
    want = MC.valid_of(oracle_mask(oracle, cam.pipe, size))
    assert np.array_equal(mask["image"], want) and 0 < int((want == 255).sum()) < want.size
    # the mask of the image actually delivered: the selected head's
    cam.pipe.set_output_size(100, 68)
    msgs = cam.on_image(frame, "mono8")
    mask = [m for m in msgs if m["topic"] == "/cam0/image_mask"][0]
    assert mask["image"].shape == msgs[0]["image"].shape == (68, 100)
    assert np.array_equal(mask["image"], cam.pipe.get_output_mask(136, 200, 1, "mono8"))
    # the pipelined path carries the frame's geometry with its ticket
    cam.pipe.set_output_size(0, 0)
    assert cam.on_image_pipelined(frame, "mono8") == []
    msgs = cam.flush()
    assert np.array_equal([m for m in msgs if m["topic"] == "/cam0/image_mask"][0]["image"], want)
    # off: the messages of before
    off = CameraStream(dict(params, rect_mask="off"), device=0)
    assert "/cam0/image_mask" not in off.topics() + [m["topic"] for m in off.on_image(frame, "mono8")]


@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade(tmp_path, oracle, branch):
    w, h = 64, 48
    exe = build_facade_program(tmp_path, branch)
    calib, out_path = tmp_path / "calib.yaml", str(tmp_path / "out.bin")
    calib.write_text(synth.calibration_yaml(synth.camera_model(w, h)))
    r = subprocess.run([exe, "gpu", str(calib), str(w), str(h), out_path], capture_output=True, text=True, env=run_env(0))
    assert r.returncode == 0 and "mask gpu OK" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(out_path, np.uint8)
    want = MC.expected(oracle, *MC.fisheye_maps(oracle, (w, h), (1.0, 1.0)), (w, h))
    assert all(v > 0 for v in MC.classes(want))
    assert np.array_equal(got[:w * h].reshape(h, w), want) and np.array_equal(got[w * h:2 * w * h].reshape(h, w), MC.valid_of(want))
    head = HC.Head(size=(w // 2, h // 2), roi=(0, 0, w, h // 2), fit="letterbox")
    assert np.array_equal(got[2 * w * h:].reshape(h // 2, w // 2), twin_delivers(want, head))


# ---- a seeded fuzz ----------------------------------------------------------------------------------------------------------------
FUZZ_CASES = 20


def fuzz_case(seed):
    rng = np.random.default_rng(77000 + seed)
    w, h = int(rng.integers(3, 260)), int(rng.integers(3, 200))
    model = ("equidistant", "plumb_bob", "rational_polynomial")[int(rng.integers(3))]
    flip = (None, 90, 180, 270)[int(rng.integers(4))]
    swap = flip in (90, 270)
    calib = (h, w) if swap else (w, h)          # the calibration has the size of the flipped image, or -- one case in four -- a larger one
    if rng.random() < 0.25:
        calib = (calib[0] + int(rng.integers(1, 40)), calib[1] + int(rng.integers(1, 40)))
    C_, R_ = calib
    roi = (0, 0, 0, 0)
    if rng.random() < 0.5:
        rw, rh = int(rng.integers(1, C_ + 1)), int(rng.integers(1, R_ + 1))
        roi = (int(rng.integers(0, C_ - rw + 1)), int(rng.integers(0, R_ - rh + 1)), rw, rh)
    size = tuple(int(v) for v in rng.integers(1, 260, 2)) if rng.random() < 0.7 else (0, 0)
    head = HC.Head(size=size, interp=("linear", "area", "linear_aa", "cubic_aa")[int(rng.integers(4))], roi=roi,
                   fit=("stretch", "letterbox", "crop")[int(rng.integers(3))], format=("native", "rgb8", "mono8")[int(rng.integers(3))])
    return dict(frame=(w, h), calib=calib, model=model, flip=flip, balance=float(rng.choice([0.0, 0.5, 1.0])), fov=float(rng.choice([0.6, 1.0, 1.3, 1.8])),
                head=head, mode=("coverage", "valid")[int(rng.integers(2))])


@pytest.mark.parametrize("seed", range(FUZZ_CASES))
def test_fuzz(oracle, seed):
    k = fuzz_case(seed)
    if k["model"] == "equidistant":
        cam = synth.camera_model(*k["calib"])
    else:
        D = (-0.28, 0.07, 0.0005, -0.0003, 0.0) if k["model"] == "plumb_bob" else (0.3, -0.1, 0.0005, -0.0003, 0.01, 0.6, -0.05, 0.005)
        cam = synth.pinhole_camera_model(*k["calib"], D)
    p = und_pipe(k["calib"], (k["balance"], k["fov"]), model=k["model"], cam=cam, flip=k["flip"], mode=k["mode"])
    w, h = k["frame"]
    head = k["head"]
    HC.apply_head(p, head)
    enc, cn = ("mono8", 1) if head.format != "rgb8" else ("bgr8", 3)
    try:
        p.query_output(h, w, cn, enc)
    except ValueError:                          # the filter's own rules refuse the draw (an upscale under area, a factor beyond 64)
        head = head._replace(interp="linear")
        HC.apply_head(p, head)
    swap = k["flip"] in (90, 270)
    src = (h, w) if swap else (w, h)
    m = oracle_mask(oracle, p, src)
    # the first expectation: the rect mask of a frame
    frame = np.full((h, w) if cn == 1 else (h, w, 3), 255, np.uint8)
    p.process(frame, enc)
    assert np.array_equal(p.get_rect_mask(), m if k["mode"] == "coverage" else MC.valid_of(m)), k
    # the second: the head's delivered mask
    want = twin_delivers(m, head)
    got = p.get_output_mask(h, w, cn, enc)
    assert np.array_equal(got, want if k["mode"] == "coverage" else MC.valid_of(want)), k


def test_the_fuzz_draws_what_it_claims():
    cases = [fuzz_case(s) for s in range(FUZZ_CASES)]
    assert {c["model"] for c in cases} == {"equidistant", "plumb_bob", "rational_polynomial"} and {c["mode"] for c in cases} == {"coverage", "valid"}
    assert {c["flip"] for c in cases} == {None, 90, 180, 270} and {c["head"].fit for c in cases} == {"stretch", "letterbox", "crop"}
    assert {c["head"].interp for c in cases} == {"linear", "area", "linear_aa", "cubic_aa"}
    assert any(c["head"].size == (0, 0) for c in cases) and any(c["head"].roi != (0, 0, 0, 0) for c in cases)
