"""Packed 10- and 12-bit Bayer frames (bayer_*10p / 12p / 10_csi2 / 12_csi2) on the MI355X, at tolerance 0 against the CPU: a
packed frame produces exactly what the bayer_*16 frame holding its unpacked samples produces under the effective range, so the
expectation is tests/raw16_reference.py expected_raw16 on tests/packed_reference.py unpack of the bytes."""
import numpy as np
import pytest

import packed_cases as PC
import packed_reference as R
import raw16_cases as G
from helpers import DUMP_NAMES, LAYOUTS, SENTINEL, assert_images_equal, cfg, configure, device_batch, normalize_minmax, prefix_cfg, read_png
from raw16_reference import expected_raw16, narrow16
from raw_image_pipeline_amd import synth

pytestmark = pytest.mark.gpu


def setup_packed(pipe, c, method, rng_range):
    """rng_range None: no range on the handle -- the format's natural one applies.  The 16-bit opt-in stays off: these names do
    not depend on it."""
    configure(pipe, c)
    pipe.set_debayer_method(method)
    pipe.set_debayer_16bit(False)
    pipe.set_debayer_16bit_range(*(rng_range or (0, 0)))


def flip_cfg(angle):
    return cfg(flip=angle != 0, flip_angle=angle)


def check_taps(pipe, t_deb, t_col, what):
    deb, col = pipe.get_dist_debayered_image(), pipe.get_dist_color_image()
    assert_images_equal(deb, t_deb.reshape(deb.shape), what + " debayered tap")
    assert_images_equal(col, t_col.reshape(col.shape), what + " colour tap")


def device_rows(packed, pitch, offset, fill):
    """One packed frame on the device as rows of ``pitch`` bytes starting ``offset`` bytes into a 4-aligned allocation whose
    other bytes hold ``fill``; the allocation ends with the last row's payload.  Returns the [1, rows, row bytes] view."""
    import torch
    rows, rb = packed.shape
    host = np.full(offset + pitch * (rows - 1) + rb, fill, np.uint8)
    np.lib.stride_tricks.as_strided(host[offset:], (rows, rb), (pitch, 1))[...] = packed
    backing = torch.from_numpy(host).cuda()
    assert backing.data_ptr() % 4 == 0
    return torch.as_strided(backing, (1, rows, rb), (pitch * rows, pitch, 1), offset)


# ---- 1. every value at every group position ---------------------------------------------------------------------------------
@pytest.mark.parametrize("method", G.METHODS)
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_every_value_at_every_group_position(gpu_pipe, oracle, layout, method):
    """128 x 128 frames that hold every sample value at every position of a group (x mod 4, x mod 2).  The colour a site samples
    passes through the demosaic, so each value reaches the narrowing unfiltered: under the natural range, and under windows of
    255 values in which the narrowing is v - black, so that no bit of a value can hide behind it.  Bilinear's border rule
    computes the outermost rows and columns at the clamped position: two more frames, rolled by a half and a quarter of the size
    (multiples of 4: Bayer phase and group position stay), bring every site inside."""
    bits, group = R.BITS[layout], R.GROUP[layout]
    n, w, h = 1 << bits, 128, 128
    rng = np.random.default_rng(bits + group)
    per = w // group * h
    assert per >= n
    base = np.empty((h, w), np.uint16)
    for pos in range(group):
        order = np.concatenate([rng.permutation(n) for _ in range(-(-per // n))])[:per]
        base[:, pos::group] = order.reshape(h, w // group)
    pos_of = np.broadcast_to(np.arange(w) % group, (h, w))
    windows = [None] + [(b, b + 255) for b in range(0, n, 255)]
    seen = {False: np.zeros((n, group), bool), True: np.zeros((n, group), bool)}
    enc = R.enc("rggb", layout)
    for window in windows:
        black, white = PC.effective_range(layout, window)
        setup_packed(gpu_pipe, cfg(), method, window)
        for shift in (0, 64, 32):
            frame = np.roll(base, (shift, shift), axis=(0, 1))
            assert np.array_equal(np.roll(pos_of, shift, axis=1), pos_of)
            got = gpu_pipe.process(R.pack(frame, layout), enc)
            assert got.dtype == np.uint8 and gpu_pipe.last_encoding == "bgr8"
            what = "all values %s %s range %s shift %d" % (layout, method, window, shift)
            assert_images_equal(got, expected_raw16(oracle, cfg(), frame, "rggb", method, black, white)[0], what)
            want = narrow16(frame, black, white)
            sampled = np.empty_like(want)
            sampled[0::2, 0::2] = got[0::2, 0::2, 2]   # rggb: R
            sampled[0::2, 1::2] = got[0::2, 1::2, 1]
            sampled[1::2, 0::2] = got[1::2, 0::2, 1]
            sampled[1::2, 1::2] = got[1::2, 1::2, 0]   # B
            inner = (slice(None), slice(None)) if method == "mht" else (slice(1, -1), slice(1, -1))
            bad = np.flatnonzero(sampled[inner] != want[inner])
            assert bad.size == 0, "%s: n(%d) = %d, expected %d (%d sites differ)" % (
                what, frame[inner].ravel()[bad[0]], sampled[inner].ravel()[bad[0]], want[inner].ravel()[bad[0]], bad.size)
            v, p = frame[inner].ravel(), pos_of[inner].ravel()
            if window is None:
                seen[False][v, p] = True
            else:   # inside the window the narrowing is the identity on v - black
                inside = (v >= black) & (v <= white)
                assert np.array_equal(want[inner].ravel()[inside], (v[inside] - black).astype(np.uint8))
                seen[True][v[inside], p[inside]] = True
    assert seen[False].all(), "%d (value, position) pairs never reached the narrowing" % int((~seen[False]).sum())
    assert seen[True].all(), "%d (value, position) pairs never came out bit for bit" % int((~seen[True]).sum())


# ---- 2. layouts x patterns x methods x flips -------------------------------------------------------------------------------
@pytest.mark.parametrize("angle", G.ANGLES)
@pytest.mark.parametrize("method", G.METHODS)
@pytest.mark.parametrize("name", R.NAMES)
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_unpack_demosaic_narrow_flip(gpu_pipe, oracle, layout, name, method, angle):
    """Every size at a tight pitch through the host path (4-aligned device rows: interior tiles load dwords) and as a resident
    frame at a 4-aligned pitch, at a pitch that is no multiple of 4 and at a pointer 1-3 bytes off (both: the byte path
    everywhere), with the pitch padding and the trailing bits of each row's last byte holding a sentinel and then its
    complement: the output may not move."""
    import torch
    c = flip_cfg(angle)
    enc = R.enc(name, layout)
    bits = R.BITS[layout]
    ranges = PC.RANGES[bits]
    for k, (w, h) in enumerate(PC.sizes(layout)):
        rng_range = ranges[(k + angle // 90) % len(ranges)]
        black, white = PC.effective_range(layout, rng_range)
        setup_packed(gpu_pipe, c, method, rng_range)
        kind = "random" if (k + angle // 90) % 2 else "scene"
        frame = PC.gen_samples(w, h, name, 10 * k + angle, layout, black, white, kind=kind)
        what = "%s %s flip %d %dx%d range %s %s" % (enc, method, angle, w, h, rng_range, kind)
        ref, _ = expected_raw16(oracle, c, frame, name, method, black, white)
        packed = R.pack(frame, layout)
        assert_images_equal(gpu_pipe.process(packed, enc), ref, what + " tight")
        assert_images_equal(gpu_pipe.process(R.pitched(packed, packed.shape[1] + 3, 0xEE)[0], enc, width=w), ref, what + " pitched host rows")
        rb = packed.shape[1]
        geometries = [("pitch4", (rb + 3) // 4 * 4 + 4, 0), ("odd pitch", (rb + 3) // 4 * 4 + 1 + k % 3, 0), ("offset", (rb + 3) // 4 * 4 + 4, 1 + k % 3)]
        for label, pitch, offset in geometries:
            outs = []
            for fill in (0, 1):
                view = device_rows(R.pack(frame, layout, fill_bits=fill), pitch, offset, 0xFF * fill ^ SENTINEL)
                outs.append(gpu_pipe.apply_device(view, enc, width=w).cpu().numpy()[0])
            assert_images_equal(outs[0], ref, what + " " + label)
            assert np.array_equal(outs[0], outs[1]), what + " " + label + ": padding bytes or trailing bits were interpreted"
    torch.cuda.synchronize()


# ---- 3. the whole chain -----------------------------------------------------------------------------------------------------
def chain_cfg(w, h, wb_method, **kw):
    base = dict(flip=True, flip_angle=180, wb=True, wb_method=wb_method, wb_temporal=wb_method == "ccc", cc=True, cc_bias=(3.0, -2.0, 1.5),
                gamma=True, gamma_k=0.8, vig=True, ce=True, ce_sat=1.2, undistort=True, cam=synth.camera_model(w, h))
    base.update(kw)
    return cfg(**base)


# one layout per bit depth through everything, the other two through one white-balance method
CHAIN_CASES = [(layout, wb) for layout in ("10p", "12_csi2") for wb in ("grey_world", "pca", "simple", "ccc")] + [("12p", "grey_world"), ("10_csi2", "ccc")]


@pytest.mark.parametrize("fp_contract", [0, 1])
@pytest.mark.parametrize("method", G.METHODS)
@pytest.mark.parametrize("layout,wb_method", CHAIN_CASES)
def test_whole_chain(gpu_pipe, oracle, layout, wb_method, method, fp_contract):
    w, h, n = 644, 482, 2
    name = "grbg"
    rng_range = (64, 1023) if R.BITS[layout] == 10 else (256, 4095)
    black, white = rng_range
    c = chain_cfg(w, h, wb_method)
    setup_packed(gpu_pipe, c, method, rng_range)
    gpu_pipe.set_fp_contraction(fp_contract)
    occ = None
    if wb_method == "ccc":
        filt, bias = synth.ccc_model()
        gpu_pipe.set_ccc_model(filt, bias)
        gpu_pipe.set_ccc_kalman_model(1.0, 10.0)
        gpu_pipe.reset_white_balance_temporal_consistency()
        occ = oracle.CCC(filt, bias)
        occ.set_kalman_model(1.0, 10.0)
    tints = [(0.70, 1.00, 0.55), (0.55, 1.00, 0.80)]
    for i in range(n):
        frame = PC.gen_samples(w, h, name, 60 + i, layout, black, white, tint=tints[i])
        what = "%s %s %s fc%d frame %d" % (layout, wb_method, method, fp_contract, i)
        got = gpu_pipe.process(R.pack(frame, layout), R.enc(name, layout))
        assert gpu_pipe.last_encoding == "bgr8"
        with oracle.fp_contraction(fp_contract):
            ref, enc, t_deb, t_col = expected_raw16(oracle, c, frame, name, method, black, white, ccc=occ, taps=True)
        assert_images_equal(got, ref, what)
        check_taps(gpu_pipe, t_deb, t_col, what)
        assert_images_equal(gpu_pipe.get_processed_image(), ref, what + " processed image")


@pytest.mark.parametrize("method", G.METHODS)
@pytest.mark.parametrize("layout", ["12p", "10_csi2"])
def test_debug_dumps(rip_lib, oracle, tmp_path, monkeypatch, layout, method):
    """The eight dumps against the oracle's chain cut after each module."""
    from raw_image_pipeline_amd import RawImagePipeline
    w, h = 160, 120
    name = "gbrg"
    black, white = R.natural_range(layout)
    monkeypatch.setenv("RIP_DEBUG_DIR", str(tmp_path))   # read when the handle is created
    pipe = RawImagePipeline(False, "", "", "", device=0)
    c = chain_cfg(w, h, "pca", flip_angle=180)
    setup_packed(pipe, c, method, None)
    pipe.set_debug(True)
    frame = PC.gen_samples(w, h, name, 90, layout, black, white)
    got = pipe.process(R.pack(frame, layout), R.enc(name, layout))
    ref, _ = expected_raw16(oracle, c, frame, name, method, black, white)
    assert_images_equal(got, ref, "final")
    for k, dump in enumerate(DUMP_NAMES):
        want, _ = expected_raw16(oracle, prefix_cfg(c, k), frame, name, method, black, white)
        assert_images_equal(read_png(str(tmp_path / (dump + ".png"))), normalize_minmax(want), dump)


# ---- 4. ranges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", G.METHODS)
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_ranges(gpu_pipe, oracle, layout, method):
    w, h, name = R.allowed_width(203, layout), 101, "bggr"
    bits = R.BITS[layout]
    top = (1 << bits) - 1
    enc = R.enc(name, layout)
    c = cfg(flip=True, flip_angle=270, gamma=True)
    frame = PC.gen_samples(w, h, name, 7, layout, 0, top, kind="random")
    packed = R.pack(frame, layout)
    setup_packed(gpu_pipe, c, method, None)
    assert gpu_pipe.get_debayer_16bit_range() == (0, 0)
    natural = gpu_pipe.process(packed, enc)
    assert natural.dtype == np.uint8 and gpu_pipe.last_encoding == "bgr8"
    assert_images_equal(natural, expected_raw16(oracle, c, frame, name, method, 0, top)[0], "natural range")
    for rng_range in [(0, top), (64, 1023) if bits == 10 else (256, 4095), (0, 65535), (top // 2, 3 * top)]:
        gpu_pipe.set_debayer_16bit_range(*rng_range)
        got = gpu_pipe.process(packed, enc)
        assert gpu_pipe.last_encoding == "bgr8" and gpu_pipe.get_debayer_16bit_range() == rng_range
        assert_images_equal(got, expected_raw16(oracle, c, frame, name, method, *rng_range)[0], "%s range %s" % (enc, rng_range))
        if rng_range == (0, top):
            assert np.array_equal(got, natural)
    # the 16-bit opt-in changes nothing for these names
    gpu_pipe.set_debayer_16bit(True)
    assert np.array_equal(gpu_pipe.process(packed, enc), got)
    # the twin: the bayer_*16 frame of the unpacked samples under the same range, same handle
    twin = gpu_pipe.process(R.unpack(packed, w, layout), G.enc16(name))
    assert np.array_equal(twin, got)


# ---- 5. resident batches --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch_layout", LAYOUTS)
@pytest.mark.parametrize("n", G.BATCHES)
def test_resident_batches(gpu_pipe, oracle, n, batch_layout):
    import torch
    k = LAYOUTS.index(batch_layout)
    layout = R.LAYOUTS[(k + n) % 4]
    method, name, angle = G.METHODS[(k + n // 2) % 2], R.NAMES[(k + n) % 4], [0, 180, 90, 270, 180][k]
    w, h = (336, 200) if n > 1 else (136, 70)   # 336 x 200: interior tiles, rows of whole dwords; 17 frames: five frame groups
    rng_range = [None, (64, 1023), (256, 4095)][n % 3]
    black, white = PC.effective_range(layout, rng_range)
    c = cfg(flip=angle != 0, flip_angle=angle, wb=True, wb_method="grey_world", cc=True, gamma=True)
    setup_packed(gpu_pipe, c, method, rng_range)
    frames = np.stack([PC.gen_samples(w, h, name, 300 + 20 * n + i, layout, black, white, kind="random" if i % 3 == 2 else "scene") for i in range(n)])
    assert len({f.tobytes() for f in frames}) == n
    packed = np.stack([R.pack(f, layout) for f in frames])
    batch = device_batch(packed, batch_layout, np.random.default_rng(n + k))
    ow, oh = (h, w) if angle in (90, 270) else (w, h)
    out = torch.full((n, oh, ow, 3), 0x5A, dtype=torch.uint8, device="cuda")
    taps = [torch.full((n, oh, ow, 3), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)] if n % 2 else [None, None]
    gpu_pipe.apply_device(batch.view, R.enc(name, layout), out=out, tap_debayered=taps[0], tap_color=taps[1], width=w)
    what = "batch n %d %s %s %s %s flip %d" % (n, batch_layout, layout, name, method, angle)
    batch.check_padding(what)
    out = out.cpu().numpy()
    for i in range(n):
        ref, _, t_deb, t_col = expected_raw16(oracle, c, frames[i], name, method, black, white, taps=True)
        assert_images_equal(out[i], ref, what + " frame %d" % i)
        if taps[0] is not None:
            assert_images_equal(taps[0][i].cpu().numpy(), t_deb.reshape(oh, ow, 3), what + " debayered tap %d" % i)
            assert_images_equal(taps[1][i].cpu().numpy(), t_col.reshape(oh, ow, 3), what + " colour tap %d" % i)
        assert_images_equal(gpu_pipe.process(packed[i], R.enc(name, layout)), out[i], what + " frame %d alone" % i)


# ---- 6. host paths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_host_paths(gpu_pipe, oracle, layout, depth):
    from raw_image_pipeline_amd.pipeline import host_alloc
    w, h = 320, 240
    name, angle = "bggr", 90
    method = G.METHODS[(R.LAYOUTS.index(layout) + depth) % 2]
    rng_range = (64, 1023) if R.BITS[layout] == 10 else (256, 4095)
    black, white = rng_range
    c = chain_cfg(w, h, "grey_world", flip_angle=angle, cam=synth.camera_model(h, w))
    setup_packed(gpu_pipe, c, method, rng_range)
    gpu_pipe.set_ring_depth(depth)
    frames = [PC.gen_samples(w, h, name, 80 + i, layout, black, white) for i in range(4)]
    packed = [R.pack(f, layout) for f in frames]
    refs = [expected_raw16(oracle, c, f, name, method, black, white, taps=True) for f in frames]
    enc = R.enc(name, layout)
    for f, (ref, _, t_deb, t_col) in zip(packed, refs):
        got = gpu_pipe.apply(f.copy(), enc)
        assert got.dtype == np.uint8
        assert_images_equal(got, ref, "apply")
        check_taps(gpu_pipe, t_deb, t_col, "apply")
        assert_images_equal(gpu_pipe.get_processed_image(), ref, "apply processed image")
    gpu_pipe.set_tap_download(3)
    for i0 in range(0, len(frames), depth):
        tickets = [(i, gpu_pipe.submit(packed[i], enc)) for i in range(i0, min(i0 + depth, len(frames)))]
        for i, t in tickets:
            got = gpu_pipe.collect(t)
            assert got.dtype == np.uint8 and gpu_pipe.last_encoding == "bgr8"
            assert_images_equal(got, refs[i][0], "submit/collect frame %d" % i)
            check_taps(gpu_pipe, refs[i][2], refs[i][3], "submit/collect frame %d" % i)
            assert_images_equal(gpu_pipe.get_processed_image(), refs[i][0], "collect processed image")
    # a pitched frame with the width spelled out, from page-locked memory (no staging copy), as a view
    pinned = host_alloc((h, packed[0].shape[1] + 5))
    pinned[...] = 0xC3
    pinned[:, :packed[0].shape[1]] = packed[0]
    t = gpu_pipe.submit(pinned, enc, width=w)
    view = gpu_pipe.collect(t, copy=False)
    assert view.dtype == np.uint8
    assert_images_equal(view, refs[0][0], "collect view")
    ref, _, t_deb, t_col = refs[1]
    out, tap_d, tap_c = host_alloc(ref.shape), host_alloc((w, h, 3)), host_alloc((w, h, 3))
    t = gpu_pipe.submit(packed[1], enc, out=out, tap_debayered=tap_d, tap_color=tap_c)
    assert gpu_pipe.collect(t) is out
    assert_images_equal(out, ref, "submit_to")
    assert_images_equal(tap_d, t_deb.reshape(tap_d.shape), "submit_to debayered tap")
    assert_images_equal(tap_c, t_col.reshape(tap_c.shape), "submit_to colour tap")


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_frontend_round_trip(rip_lib, oracle, layout):
    """on_image and the pipelined callback of the front end on packed frames, levels from the node parameters."""
    from raw_image_pipeline_amd import RawImagePipeline
    from raw_image_pipeline_amd.frontend import CameraStream
    w, h, name = 160, 96, "rggb"
    black, white = (64, 1023) if R.BITS[layout] == 10 else (256, 4095)
    cam = CameraStream({"debayer/black_level": black, "debayer/white_level": white, "output_encoding": "passthrough"},
                       pipeline=RawImagePipeline(False, "", "", "", device=0))
    c = cfg()
    configure(cam.pipe, c)
    frames = [PC.gen_samples(w, h, name, 40 + i, layout, black, white) for i in range(2)]
    refs = [expected_raw16(oracle, c, f, name, "bilinear", black, white)[0] for f in frames]
    enc = R.enc(name, layout)
    def final(msgs):
        picked = [m for m in msgs if m["topic"].endswith("/" + cam.input_type + "/image")]
        assert len(picked) == 1 and picked[0]["encoding"] == "bgr8", [m["topic"] for m in msgs]
        return np.asarray(picked[0]["image"])

    assert_images_equal(final(cam.on_image(R.pack(frames[0], layout), enc)), refs[0], "on_image")
    wide = R.pitched(R.pack(frames[1], layout), R.row_bytes(w, layout) + 8, 0x11)[1]
    assert_images_equal(final(cam.on_image(wide, enc, width=w)), refs[1], "on_image with a width")
    assert cam.on_image_pipelined(R.pack(frames[0], layout), enc) == []
    assert_images_equal(final(cam.on_image_pipelined(wide, enc, width=w)), refs[0], "pipelined frame 0")
    assert_images_equal(final(cam.flush()), refs[1], "pipelined frame 1")


# ---- 7. ccc sequence against the twin 16-bit sequence -------------------------------------------------------------------------------
@pytest.mark.parametrize("method", G.METHODS)
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_ccc_sequence_equals_the_twin_16bit_sequence(rip_lib, oracle, layout, method):
    """Ten frames with a drifting tint through a packed handle and through a twin handle fed the unpacked samples as bayer_*16:
    the raw and the Kalman-filtered (u, v) of every frame, its gains and its pixels are equal, as one resident batch and as
    single calls; the pixels also equal the oracle's."""
    import torch
    from raw_image_pipeline_amd import RawImagePipeline
    w, h, n = 384, 240, 10
    name = "gbrg"
    black, white = (64, 1023) if R.BITS[layout] == 10 else (100, 4095)
    filt, bias = synth.ccc_model()
    c = cfg(wb=True, wb_method="ccc", wb_bright=0.8, wb_dark=0.2, wb_temporal=True, ce=True, ce_sat=1.2)
    frames = np.stack([PC.gen_samples(w, h, name, 2000 + i, layout, black, white, tint=(0.70 + 0.10 * i / (n - 1), 1.0, 0.55)) for i in range(n)])
    packed = np.stack([R.pack(f, layout) for f in frames])
    pipes = [RawImagePipeline(False, "", "", "", device=0) for _ in range(2)]
    for p in pipes:
        p.set_undistortion(False)
        p.set_ccc_model(filt, bias)
        p.set_ccc_kalman_model(1.0, 10.0)
        configure(p, c)
        p.set_debayer_method(method)
        p.set_debayer_16bit_range(black, white)
    pk, tw = pipes
    tw.set_debayer_16bit(True)
    occ = oracle.CCC(filt, bias)
    occ.set_kalman_model(1.0, 10.0)
    refs = [expected_raw16(oracle, c, frames[i], name, method, black, white, ccc=occ)[0] for i in range(n)]
    # (a) one resident batch each
    for p in pipes:
        p.reset_white_balance_temporal_consistency()
    out_pk = pk.apply_device(torch.from_numpy(packed).cuda(), R.enc(name, layout))
    out_tw = tw.apply_device(torch.from_numpy(frames.view(np.uint8).reshape(n, h, w * 2)).cuda(), G.enc16(name))
    torch.cuda.synchronize()
    track = pk.get_ccc_track(n)
    assert np.array_equal(track, tw.get_ccc_track(n)), "batch: the (u, v) sequences differ"
    assert len({tuple(t[2:]) for t in track}) >= 2, "the filtered estimate must follow the drift (else the test shows nothing)"
    assert np.array_equal(pk.get_white_balance_info(n), tw.get_white_balance_info(n)), "batch: white-balance info differs"
    assert torch.equal(out_pk, out_tw)
    out_pk = out_pk.cpu().numpy()
    for i in range(n):
        assert_images_equal(out_pk[i], refs[i], "ccc %s %s batch frame %d" % (layout, method, i))
    # (b) single calls
    for p in pipes:
        p.reset_white_balance_temporal_consistency()
    for i in range(n):
        got = pk.process(packed[i], R.enc(name, layout))
        twin = tw.process(frames[i], G.enc16(name))
        assert np.array_equal(got, twin), "single calls: frame %d differs from its twin" % i
        # (the reset keeps the filter's error covariance, so this pass need not repeat the batch's filtered track: the twin is
        # the reference here)
        assert np.array_equal(pk.get_ccc_track(1), tw.get_ccc_track(1)), "single calls: frame %d (u, v) differs from its twin" % i
        assert np.array_equal(pk.get_white_balance_info(1), tw.get_white_balance_info(1))


# ---- 8. seeded fuzz ---------------------------------------------------------------------------------------------------------------
COMPARED = []


@pytest.mark.parametrize("seed", range(PC.N_FUZZ))
def test_random_packed_configuration(gpu_pipe, oracle, seed):
    import torch
    case = PC.fuzz_case(seed)
    w, h, name, layout, method, c, n = (case[k] for k in ("w", "h", "name", "layout", "method", "c", "n"))
    black, white = PC.effective_range(layout, case["range"])
    what = PC.describe(case)
    enc = R.enc(name, layout)
    setup_packed(gpu_pipe, c, method, case["range"])
    frame = PC.gen_samples(w, h, name, seed, layout, black, white, kind=case["kind"], tint=case["tint"])
    got = gpu_pipe.process(R.pack(frame, layout, fill_bits=seed % 2), enc)
    assert gpu_pipe.last_encoding == "bgr8"
    ref, _, t_deb, t_col = expected_raw16(oracle, c, frame, name, method, black, white, taps=True)
    assert_images_equal(got, ref, what)
    check_taps(gpu_pipe, t_deb, t_col, what)
    frames = np.stack([PC.gen_samples(w, h, name, 1000 * seed + 7 + i, layout, black, white, kind=case["kind"] if i % 3 else "random") for i in range(n)])
    packed = np.stack([R.pack(f, layout, fill_bits=(seed + i) % 2) for i, f in enumerate(frames)])
    batch = device_batch(packed, case["batch_layout"], np.random.default_rng(case["layout_seed"]))
    aligned = batch.offset % 4 == 0 and batch.pitch % 4 == 0 and batch.frame_stride % 4 == 0
    assert (case["path"] == "interior") == (aligned and PC.has_interior_tiles(w, h)), what
    ow, oh = (h, w) if case["flip"] in (90, 270) else (w, h)
    tap = torch.full((n, oh, ow, 3), 0x5A, dtype=torch.uint8, device="cuda") if case["tap"] else None
    out = gpu_pipe.apply_device(batch.view, enc, tap_debayered=tap, width=w)
    batch.check_padding(what)
    out = out.cpu().numpy()
    for i in range(n):
        ref, _, t_deb, _ = expected_raw16(oracle, c, frames[i], name, method, black, white, taps=True)
        assert_images_equal(out[i], ref, what + " batch frame %d/%d" % (i, n))
        if tap is not None:
            assert_images_equal(tap[i].cpu().numpy(), t_deb.reshape(oh, ow, 3), what + " debayered tap of batch frame %d/%d" % (i, n))
    COMPARED.append(seed)


def test_the_fuzz_compared_every_case():
    """Runs after the cases above (file order): none of them may have been skipped or have left before its last comparison."""
    assert sorted(COMPARED) == list(range(PC.N_FUZZ)), "compared %d of %d cases" % (len(COMPARED), PC.N_FUZZ)


# ---- errors that need a device ------------------------------------------------------------------------------------------------
def test_device_calls_reject_a_pitch_below_a_row(gpu_pipe):
    import ctypes as C
    import torch
    setup_packed(gpu_pipe, cfg(), "bilinear", None)
    buf = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(16 * 16 * 3, dtype=torch.uint8, device="cuda")
    for enc, need in (("bayer_rggb10p", 20), ("bayer_rggb12_csi2", 24)):
        with pytest.raises(ValueError, match="pitch smaller than a row"):
            gpu_pipe._call("rip_apply_device", C.c_void_p(buf.data_ptr()), C.c_size_t(need - 1), C.c_size_t(0), 1, 16, 16, 1, enc.encode(),
                           C.c_void_p(out.data_ptr()), C.c_size_t(0), C.c_size_t(0), None, None)
        host = np.zeros((16, need), np.uint8)
        res = np.zeros((16, 16, 3), np.uint8)
        r, cc, k = C.c_int(), C.c_int(), C.c_int()
        with pytest.raises(ValueError, match="pitch smaller than a row"):
            gpu_pipe._call("rip_apply", host.ctypes.data_as(C.c_void_p), 16, 16, 1, C.c_size_t(need - 1), enc.encode(), res.ctypes.data_as(C.c_void_p),
                           C.c_size_t(res.nbytes), C.byref(r), C.byref(cc), C.byref(k), None)


# ---- the C++ facade on frames -------------------------------------------------------------------------------------------------
def test_cpp_facade_processes_packed_mats(tmp_path, rip_lib):
    """tests/cpp/packed_test.cpp with a device: one-channel uint8 Mats of rows x row bytes in the four layouts through apply /
    process / submit + collect / submitTo, tight and with padding columns (setDebayerPackedWidth), both methods, flip 90."""
    import os
    import subprocess
    from test_packed import build_cpp
    exe = build_cpp(tmp_path)
    env = dict(os.environ)
    env["RIP_DEVICE"] = "0"
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe, "frames"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "packed frames OK" in r.stdout and "packed facade OK" in r.stdout
