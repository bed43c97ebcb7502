"""16-bit Bayer frames through the whole chain (rip_set_debayer_16bit + rip_set_debayer_16bit_range) on the MI355X, at tolerance 0
against the CPU: the oracle run on the narrowed 16-bit demosaic (tests/raw16_reference.py expected_raw16)."""
import numpy as np
import pytest

import raw16_cases as G
from helpers import DUMP_NAMES, LAYOUTS, SENTINEL, assert_images_equal, cfg, configure, device_batch, normalize_minmax, prefix_cfg, read_png
from mht_reference import flip as np_flip
from raw16_reference import demosaic16, expected_raw16, narrow16
from raw_image_pipeline_amd import RipAssertError, synth

pytestmark = pytest.mark.gpu


def setup16(pipe, c, method, black, white):
    configure(pipe, c)
    pipe.set_debayer_method(method)
    pipe.set_debayer_16bit(True)
    pipe.set_debayer_16bit_range(black, white)


def flip_cfg(angle):
    return cfg(flip=angle != 0, flip_angle=angle)


def bytes_of(frames):
    """[n, rows, cols] uint16 -> the uint8 view [n, rows, cols * 2] of its rows."""
    frames = np.ascontiguousarray(frames, np.uint16)
    return frames.view(np.uint8).reshape(frames.shape[0], frames.shape[1], frames.shape[2] * 2)


def check_taps(pipe, t_deb, t_col, what):
    deb, col = pipe.get_dist_debayered_image(), pipe.get_dist_color_image()
    assert_images_equal(deb, t_deb.reshape(deb.shape), what + " debayered tap")
    assert_images_equal(col, t_col.reshape(col.shape), what + " colour tap")


# ---- 1. every value through the narrowing ---------------------------------------------------------------------------------
@pytest.mark.parametrize("method", G.METHODS)
@pytest.mark.parametrize("black,white", G.RANGES)
def test_every_value_through_the_narrowing(gpu_pipe, oracle, black, white, method):
    """A 256 x 256 frame holding each uint16 value once: the colour a site samples passes through the demosaic, so each value
    reaches n() unfiltered."""
    base = np.random.default_rng(black + white).permutation(65536).astype(np.uint16).reshape(256, 256)
    setup16(gpu_pipe, cfg(), method, black, white)
    seen = np.zeros(65536, bool)
    # bilinear's border rule computes the outermost rows and columns at the clamped position, so their own samples do not pass
    # through: two more frames, rolled by a half and a quarter of the size (even amounts: the Bayer phase stays), bring every
    # one of them inside
    for frame in (base, np.roll(base, (128, 128), axis=(0, 1)), np.roll(base, (64, 64), axis=(0, 1))):
        got = gpu_pipe.process(frame, "bayer_rggb16")
        assert got.dtype == np.uint8 and gpu_pipe.last_encoding == "bgr8"
        ref, enc = expected_raw16(oracle, cfg(), frame, "rggb", method, black, white)
        assert enc == "bgr8"
        assert_images_equal(got, ref, "all values %s (%d, %d)" % (method, black, white))
        n = narrow16(frame, black, white)
        sampled = np.empty_like(n)
        sampled[0::2, 0::2] = got[0::2, 0::2, 2]   # rggb: R
        sampled[0::2, 1::2] = got[0::2, 1::2, 1]
        sampled[1::2, 0::2] = got[1::2, 0::2, 1]
        sampled[1::2, 1::2] = got[1::2, 1::2, 0]   # B
        inner = (slice(None), slice(None)) if method == "mht" else (slice(1, -1), slice(1, -1))
        bad = np.flatnonzero(sampled[inner] != n[inner])
        assert bad.size == 0, "n(%d) = %d, expected %d (%d values differ)" % (frame[inner].ravel()[bad[0]], sampled[inner].ravel()[bad[0]], n[inner].ravel()[bad[0]], bad.size)
        seen[frame[inner].ravel()] = True
    assert seen.all(), "%d values never reached the narrowing unfiltered" % int((~seen).sum())


# ---- 2. demosaic + narrow + flip -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angle", G.ANGLES)
@pytest.mark.parametrize("method", G.METHODS)
@pytest.mark.parametrize("name", G.NAMES)
def test_demosaic_narrow_flip(gpu_pipe, oracle, name, method, angle):
    c = flip_cfg(angle)
    for k, (w, h) in enumerate(G.EDGE_SIZES):
        black, white = [(64, 1023), (256, 4095), (0, 65535), (1000, 60000)][(k + angle // 90) % 4]
        setup16(gpu_pipe, c, method, black, white)
        for kind in ("scene", "random"):
            frame = G.gen_frame16(w, h, name, 10 * k + angle, black, white, kind=kind)
            assert kind == "random" or (frame.min() <= black and frame.max() >= white)
            what = "%s %s flip %d %dx%d (%d, %d) %s" % (name, method, angle, w, h, black, white, kind)
            ref, _ = expected_raw16(oracle, c, frame, name, method, black, white)
            assert_images_equal(gpu_pipe.process(frame, G.enc16(name)), ref, what)
            # pitched input: rows of a wider array, pitch not a multiple of 4
            wide = np.full((h, w + 3), 0xBEEF, np.uint16)
            wide[:, :w] = frame
            assert_images_equal(gpu_pipe.process(wide[:, :w], G.enc16(name)), ref, what + " pitched")


# ---- 3. the whole chain ----------------------------------------------------------------------------------------------------
def chain_cfg(w, h, wb_method, **kw):
    base = dict(flip=True, flip_angle=180, wb=True, wb_method=wb_method, wb_temporal=wb_method == "ccc", cc=True, cc_bias=(3.0, -2.0, 1.5),
                gamma=True, gamma_k=0.8, vig=True, ce=True, ce_sat=1.2, undistort=True, cam=synth.camera_model(w, h))
    base.update(kw)
    return cfg(**base)


@pytest.mark.parametrize("fp_contract", [0, 1])
@pytest.mark.parametrize("method", G.METHODS)
@pytest.mark.parametrize("wb_method", ["grey_world", "pca", "simple", "ccc"])
def test_whole_chain(gpu_pipe, oracle, wb_method, method, fp_contract):
    w, h, n = 644, 482, 2
    name, black, white = "grbg", 200, 4000
    c = chain_cfg(w, h, wb_method)
    setup16(gpu_pipe, c, method, black, white)
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
        frame = G.gen_frame16(w, h, name, 60 + i, black, white, tint=tints[i])
        what = "%s %s fc%d frame %d" % (wb_method, method, fp_contract, i)
        got = gpu_pipe.process(frame, G.enc16(name))
        assert gpu_pipe.last_encoding == "bgr8"
        with oracle.fp_contraction(fp_contract):
            ref, enc, t_deb, t_col = expected_raw16(oracle, c, frame, name, method, black, white, ccc=occ, taps=True)
        assert_images_equal(got, ref, what)
        check_taps(gpu_pipe, t_deb, t_col, what)
        assert_images_equal(gpu_pipe.get_processed_image(), ref, what + " processed image")
        # DEBAYERED = the flipped narrowed image
        assert_images_equal(gpu_pipe.get_dist_debayered_image(), np_flip(narrow16(demosaic16(oracle, frame, name, method), black, white), 180), what + " N")


# ---- 4. resident batches ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_taps", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [1, 3, 17])
def test_resident_batches(gpu_pipe, oracle, n, layout, with_taps):
    import torch
    k = LAYOUTS.index(layout)
    method, name, angle = G.METHODS[(k + n) % 2], G.NAMES[(k + n) % 4], [0, 180, 90, 270, 180][k]
    w, h = (328, 200) if n > 1 else (136, 70)   # 328 x 200: interior tiles; 17 frames: five frame groups
    black, white = 64, 1023
    c = cfg(flip=angle != 0, flip_angle=angle, wb=True, wb_method="grey_world", cc=True, gamma=True)
    setup16(gpu_pipe, c, method, black, white)
    frames = np.stack([G.gen_frame16(w, h, name, 300 + 20 * n + i, black, white, kind="random" if i % 3 == 2 else "scene") for i in range(n)])
    assert len({f.tobytes() for f in frames}) == n
    batch = device_batch(bytes_of(frames), layout, np.random.default_rng(n + k))
    ow, oh = (h, w) if angle in (90, 270) else (w, h)
    out = torch.full((n, oh, ow, 3), 0x5A, dtype=torch.uint8, device="cuda")
    taps = [torch.full((n, oh, ow, 3), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)] if with_taps else [None, None]
    gpu_pipe.apply_device(batch.view, G.enc16(name), out=out, tap_debayered=taps[0], tap_color=taps[1])
    what = "batch n %d %s taps %d %s %s flip %d" % (n, layout, with_taps, name, method, angle)
    batch.check_padding(what)
    out = out.cpu().numpy()
    for i in range(n):
        ref, _, t_deb, t_col = expected_raw16(oracle, c, frames[i], name, method, black, white, taps=True)
        assert_images_equal(out[i], ref, what + " frame %d" % i)
        if with_taps:
            assert_images_equal(taps[0][i].cpu().numpy(), t_deb.reshape(oh, ow, 3), what + " debayered tap %d" % i)
            assert_images_equal(taps[1][i].cpu().numpy(), t_col.reshape(oh, ow, 3), what + " colour tap %d" % i)
        # each frame equal to its single-frame result
        assert_images_equal(gpu_pipe.process(frames[i], G.enc16(name)), out[i], what + " frame %d alone" % i)


# ---- 5. host paths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("method", G.METHODS)
def test_host_paths(gpu_pipe, oracle, method, depth):
    from raw_image_pipeline_amd.pipeline import host_alloc
    w, h = 320, 240
    name, black, white, angle = "bggr", 256, 4095, 90
    c = chain_cfg(w, h, "grey_world", flip_angle=angle, cam=synth.camera_model(h, w))
    setup16(gpu_pipe, c, method, black, white)
    gpu_pipe.set_ring_depth(depth)
    frames = [G.gen_frame16(w, h, name, 80 + i, black, white) for i in range(4)]
    refs = [expected_raw16(oracle, c, f, name, method, black, white, taps=True) for f in frames]
    enc = G.enc16(name)
    # rip_apply (apply() cannot re-seat a uint16 array with a uint8 image of another shape: it returns it)
    for f, (ref, _, t_deb, t_col) in zip(frames, refs):
        got = gpu_pipe.apply(f.copy(), enc)
        assert got.dtype == np.uint8
        assert_images_equal(got, ref, "apply")
        check_taps(gpu_pipe, t_deb, t_col, "apply")
        assert_images_equal(gpu_pipe.get_processed_image(), ref, "apply processed image")
    # rip_submit / rip_collect with as many frames in flight as the ring holds, taps downloaded with the result
    gpu_pipe.set_tap_download(3)
    for i0 in range(0, len(frames), depth):
        tickets = [(i, gpu_pipe.submit(frames[i], enc)) for i in range(i0, min(i0 + depth, len(frames)))]
        for i, t in tickets:
            got = gpu_pipe.collect(t)
            assert got.dtype == np.uint8 and gpu_pipe.last_encoding == "bgr8"
            assert_images_equal(got, refs[i][0], "submit/collect frame %d" % i)
            check_taps(gpu_pipe, refs[i][2], refs[i][3], "submit/collect frame %d" % i)
            assert_images_equal(gpu_pipe.get_processed_image(), refs[i][0], "collect processed image")
    t = gpu_pipe.submit(frames[0], enc)
    view = gpu_pipe.collect(t, copy=False)
    assert view.dtype == np.uint8
    assert_images_equal(view, refs[0][0], "collect view")
    # rip_submit_to into page-locked uint8 arrays of the caller
    ref, _, t_deb, t_col = refs[1]
    out, tap_d, tap_c = host_alloc(ref.shape), host_alloc((w, h, 3)), host_alloc((w, h, 3))
    assert out.dtype == np.uint8
    t = gpu_pipe.submit(frames[1], enc, out=out, tap_debayered=tap_d, tap_color=tap_c)
    assert gpu_pipe.collect(t) is out
    assert_images_equal(out, ref, "submit_to")
    assert_images_equal(tap_d, t_deb.reshape(tap_d.shape), "submit_to debayered tap")
    assert_images_equal(tap_c, t_col.reshape(tap_c.shape), "submit_to colour tap")


def test_output_pool_hands_out_uint8(gpu_pipe, oracle):
    from raw_image_pipeline_amd.pipeline import OutputPool
    w, h, name = 64, 48, "rggb"
    setup16(gpu_pipe, cfg(gamma=True), "bilinear", 0, 4095)
    gpu_pipe.out_pool = OutputPool(limit=4, pinned=True)
    frame = G.gen_frame16(w, h, name, 5, 0, 4095)
    ref, _ = expected_raw16(oracle, cfg(gamma=True), frame, name, "bilinear", 0, 4095)
    for _ in range(3):
        got = gpu_pipe.process(frame, G.enc16(name))
        assert got.dtype == np.uint8
        assert_images_equal(got, ref, "pool process")
        got = gpu_pipe.collect(gpu_pipe.submit(frame, G.enc16(name)))
        assert got.dtype == np.uint8
        assert_images_equal(got, ref, "pool collect")
        del got


@pytest.mark.parametrize("method", G.METHODS)
def test_debug_dumps(rip_lib, oracle, tmp_path, monkeypatch, method):
    """The eight dumps against the oracle's chain cut after each module."""
    from raw_image_pipeline_amd import RawImagePipeline
    w, h = 160, 120
    name, black, white = "gbrg", 64, 1023
    monkeypatch.setenv("RIP_DEBUG_DIR", str(tmp_path))   # read when the handle is created
    pipe = RawImagePipeline(False, "", "", "", device=0)
    c = chain_cfg(w, h, "pca", flip_angle=180)
    setup16(pipe, c, method, black, white)
    pipe.set_debug(True)
    frame = G.gen_frame16(w, h, name, 90, black, white)
    got = pipe.process(frame, G.enc16(name))
    ref, _ = expected_raw16(oracle, c, frame, name, method, black, white)
    assert_images_equal(got, ref, "final")
    for k, dump in enumerate(DUMP_NAMES):
        want, _ = expected_raw16(oracle, prefix_cfg(c, k), frame, name, method, black, white)
        assert_images_equal(read_png(str(tmp_path / (dump + ".png"))), normalize_minmax(want), dump)


# ---- 6. ccc sequence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", G.METHODS)
def test_ccc_sequence_with_temporal_consistency(gpu_pipe, oracle, method):
    """Ten frames with a drifting tint: the raw and the Kalman-filtered (u, v) of every frame, its gains and its pixels, as single
    calls and as one resident batch, against one oracle filter state walked through the narrowed images."""
    import torch
    w, h, n = 384, 240, 10
    name, black, white = "gbrg", 100, 16383
    filt, bias = synth.ccc_model()
    c = cfg(wb=True, wb_method="ccc", wb_bright=0.8, wb_dark=0.2, wb_temporal=True, ce=True, ce_sat=1.2)
    frames = np.stack([G.gen_frame16(w, h, name, 2000 + i, black, white, tint=(0.70 + 0.10 * i / (n - 1), 1.0, 0.55)) for i in range(n)])
    occ_track = oracle.CCC(filt, bias)
    occ_track.set_thresholds(0.8, 0.2)
    occ_track.set_temporal_consistency(True)
    occ_track.set_kalman_model(1.0, 10.0)
    occ_pixels = oracle.CCC(filt, bias)
    occ_pixels.set_kalman_model(1.0, 10.0)

    def oracle_pass():
        track, gains, refs = [], [], []
        for i in range(n):
            _, info, g = occ_track.balance(narrow16(demosaic16(oracle, frames[i], name, method), black, white))
            track.append(info)
            gains.append(g)
            refs.append(expected_raw16(oracle, c, frames[i], name, method, black, white, ccc=occ_pixels)[0])
        return np.asarray(track, np.int32), np.asarray(gains, np.float32), refs

    track, gains, refs = oracle_pass()
    assert len({tuple(t[2:]) for t in track}) >= 2, "the filtered estimate must follow the drift (else the test shows nothing)"
    gpu_pipe.set_ccc_model(filt, bias)
    gpu_pipe.set_ccc_kalman_model(1.0, 10.0)
    setup16(gpu_pipe, c, method, black, white)
    # (a) one resident batch
    gpu_pipe.reset_white_balance_temporal_consistency()
    out = gpu_pipe.apply_device(torch.from_numpy(bytes_of(frames)).cuda(), G.enc16(name))
    torch.cuda.synchronize()
    got_track = gpu_pipe.get_ccc_track(n)
    assert np.array_equal(got_track, track), "batch: (u, v) sequence differs first at frame %d" % int(np.argmax((got_track != track).any(axis=1)))
    assert np.array_equal(gpu_pipe.get_white_balance_info(n)[:, 0:3], gains), "batch: gains differ"
    out = out.cpu().numpy()
    for i in range(n):
        assert_images_equal(out[i], refs[i], "ccc %s batch frame %d" % (method, i))
    # (b) single calls; the reset keeps the error covariance on both sides
    gpu_pipe.reset_white_balance_temporal_consistency()
    occ_track.reset()
    occ_pixels.reset()
    track, gains, refs = oracle_pass()
    for i in range(n):
        got = gpu_pipe.process(frames[i], G.enc16(name))
        t = gpu_pipe.get_ccc_track(1)[0]
        assert np.array_equal(t, track[i]), "single calls: frame %d (u, v) %s, oracle %s" % (i, t, track[i])
        assert np.array_equal(gpu_pipe.get_white_balance_info(1)[0][0:3], gains[i])
        assert_images_equal(got, refs[i], "ccc %s single call frame %d" % (method, i))


# ---- 7. seeded fuzz ------------------------------------------------------------------------------------------------------------
COMPARED = []


@pytest.mark.parametrize("seed", range(G.N_FUZZ))
def test_random_raw16_configuration(gpu_pipe, oracle, seed):
    import torch
    case = G.fuzz_case(seed)
    w, h, name, method, black, white, c, n = (case[k] for k in ("w", "h", "name", "method", "black", "white", "c", "n"))
    what = G.describe(case)
    setup16(gpu_pipe, c, method, black, white)
    frame = G.gen_frame16(w, h, name, seed, black, white, kind=case["kind"], tint=case["tint"])
    got = gpu_pipe.process(frame, G.enc16(name))
    assert gpu_pipe.last_encoding == "bgr8"
    ref, enc, t_deb, t_col = expected_raw16(oracle, c, frame, name, method, black, white, taps=True)
    assert_images_equal(got, ref, what)
    check_taps(gpu_pipe, t_deb, t_col, what)
    frames = np.stack([G.gen_frame16(w, h, name, 1000 * seed + 7 + i, black, white, kind=case["kind"] if i % 3 else "random") for i in range(n)])
    batch = device_batch(bytes_of(frames), case["layout"], np.random.default_rng(case["layout_seed"]))
    ow, oh = (h, w) if case["flip"] in (90, 270) else (w, h)
    tap = torch.full((n, oh, ow, 3), 0x5A, dtype=torch.uint8, device="cuda") if case["tap"] else None
    out = gpu_pipe.apply_device(batch.view, G.enc16(name), tap_debayered=tap)
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
    assert sorted(COMPARED) == list(range(G.N_FUZZ)), "compared %d of %d cases" % (len(COMPARED), G.N_FUZZ)


# ---- 8. unchanged behaviour ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", G.METHODS)
def test_range_off_again_is_todays_bgr16(gpu_pipe, oracle, method):
    from mht_reference import mht_reference
    w, h, angle = 131, 67, 180
    frame = np.random.default_rng(3).integers(0, 65536, (h, w)).astype(np.uint16)
    configure(gpu_pipe, flip_cfg(angle))
    gpu_pipe.set_debayer_method(method)
    gpu_pipe.set_debayer_16bit(True)
    gpu_pipe.set_taps(7)
    before = gpu_pipe.process(frame, "bayer_gbrg16")
    assert before.dtype == np.uint16 and gpu_pipe.last_encoding == "bgr16"
    gpu_pipe.set_debayer_16bit_range(64, 1023)
    on = gpu_pipe.process(frame, "bayer_gbrg16")
    assert on.dtype == np.uint8 and gpu_pipe.last_encoding == "bgr8"
    assert_images_equal(on, expected_raw16(oracle, flip_cfg(angle), frame, "gbrg", method, 64, 1023)[0], "range on")
    gpu_pipe.set_debayer_16bit_range(0, 0)
    after = gpu_pipe.process(frame, "bayer_gbrg16")
    assert after.dtype == np.uint16 and gpu_pipe.last_encoding == "bgr16"
    assert np.array_equal(after, before)
    d16 = mht_reference(frame, "gbrg") if method == "mht" else oracle.debayer16(frame, "bayer_gbrg16")
    assert np.array_equal(after, np_flip(d16, angle))
    assert gpu_pipe.get_dist_debayered_image().size == 0   # no taps, as before
    gpu_pipe.set_gamma_correction(True)
    with pytest.raises(RipAssertError):
        gpu_pipe.process(frame, "bayer_gbrg16")
    gpu_pipe.set_debayer_16bit_range(64, 1023)   # ... and with the range the same stage set runs
    assert gpu_pipe.process(frame, "bayer_gbrg16").dtype == np.uint8


# ---- the C++ facade on frames -------------------------------------------------------------------------------------------------
def test_cpp_facade_processes_16bit_mats(tmp_path, rip_lib):
    """tests/cpp/raw16_test.cpp with a device: a one-channel Mat of 16-bit samples through apply / process / submit + collect /
    submitTo comes back as a uint8 bgr8 Mat, both methods, flip 90."""
    import os
    import subprocess
    from test_raw16 import build_cpp
    exe = build_cpp(tmp_path)
    env = dict(os.environ)
    env["RIP_DEVICE"] = "0"
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe, "frames"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "raw16 frames OK" in r.stdout and "raw16 range OK" in r.stdout
