"""The pinhole distortion models (plumb_bob, radtan, rational_polynomial) on the MI355X, at tolerance 0: the maps the device
builds (rip_maps.hip pinhole_maps_kernel) against the host builder and tests/pinhole_reference.py, and whole frames through
every remap path against the CPU oracle run on the reference maps.  Every frame test first asserts on its own maps that at
least half of the destination samples inside the source (and, at balance 1, at least 3 % outside)."""
import functools

import numpy as np
import pytest

import pinhole_reference as PR
from helpers import LAYOUTS, assert_images_equal, cfg, configure, device_batch, oracle_params, oracle_run
from raw_image_pipeline_amd import synth

pytestmark = pytest.mark.gpu

NAMES = sorted(PR.CALIBRATIONS)
FRAME_SIZES = ((200, 136), (328, 200))


def new_pipe():
    from raw_image_pipeline_amd import RawImagePipeline
    return RawImagePipeline(False, "", "", "", device=0)


@functools.lru_cache(maxsize=None)
def reference(name, size, balance):
    """(cam, model, map_x, map_y) of a calibration, from the reference alone: its new camera matrix, its maps.  Computed once
    and shared; the arrays are read-only."""
    model, D = PR.CALIBRATIONS[name]
    cam = synth.pinhole_camera_model(size[0], size[1], D)
    newK = PR.new_camera_matrix(cam["K"], model, D, size, balance)
    mx, my = PR.maps(cam["K"], model, D, cam["R"], newK, size)
    PR.check_map_conditions(mx, my, size, balance, "%s %s balance %g" % (name, size, balance))
    mx, my = np.ascontiguousarray(mx), np.ascontiguousarray(my)
    mx.setflags(write=False)
    my.setflags(write=False)
    return cam, model, mx, my


@functools.lru_cache(maxsize=None)
def bayer_frame(size, seed=21):
    f = synth.gen_frame(size[0], size[1], "bayer_rggb8", seed=seed, kind="scene")
    f.setflags(write=False)
    return f


def setup(pipe, c, name, size, balance):
    """Configuration c (without a camera: helpers.configure would load it as equidistant) and calibration `name`."""
    assert c["cam"] is None
    configure(pipe, c)
    PR.load(pipe, name, size, balance)
    return reference(name, size, balance)


def expected(O, c, frame, encoding, mx, my, taps=False):
    """What helpers.oracle_run returns, with the undistortion reading the given maps."""
    keep = []
    prm = oracle_params(O, c, keep)  # c carries no camera: no fisheye maps
    prm.und_enabled = 1
    prm.map_x, prm.map_y = mx.ctypes.data, my.ctypes.data
    prm.map_rows, prm.map_cols = mx.shape
    return O.pipeline(prm, np.ascontiguousarray(frame), encoding, taps=taps)


# ---- maps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_device_maps_equal_host_maps_and_the_reference(rip_lib, monkeypatch, name):
    """One device handle and its RIP_MAPS_ON_HOST twin walk every size and balance: the same floats from pinhole_maps_kernel,
    from rip_host.cpp and from the reference, and the same remap plan from the device and the host compiler."""
    dev = new_pipe()
    monkeypatch.setenv("RIP_MAPS_ON_HOST", "1")
    twin = new_pipe()
    monkeypatch.delenv("RIP_MAPS_ON_HOST")
    for size in PR.MAP_SIZES + ((328, 200),):
        for balance in (0.0, 0.5, 1.0):
            what = "%s %s balance %g" % (name, size, balance)
            cam, model = PR.load(dev, name, size, balance)
            PR.load(twin, name, size, balance)
            assert np.array_equal(dev.get_rect_camera_matrix(), twin.get_rect_camera_matrix())
            info_d, info_h = dev.debug_plan_info(size[1], size[0]), twin.debug_plan_info(size[1], size[0])
            assert info_d["on_device"] == 1 and info_h["on_device"] == 0, what
            for key in ("tiles_x", "tiles_y", "border_pixels", "max_lds_bytes", "max_rect_w", "max_rect_h"):
                assert info_d[key] == info_h[key], (what, key, info_d, info_h)
            mx, my = dev.get_undistortion_maps()
            hx, hy = twin.get_undistortion_maps()
            assert np.array_equal(mx, hx) and np.array_equal(my, hy), what
            rx, ry = PR.reference_maps(dev, cam, model)
            assert np.array_equal(mx, rx) and np.array_equal(my, ry), what
            assert np.array_equal(dev.get_rect_camera_matrix(), PR.new_camera_matrix(cam["K"], model, cam["D"], size, balance)), what


# ---- frames through every remap path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", FRAME_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("balance", (0.0, 1.0))
@pytest.mark.parametrize("name", NAMES)
def test_frames_equal_the_oracle_on_reference_maps(oracle, name, balance, size):
    from raw_image_pipeline_amd import TAP_COLOR, TAP_DEBAYERED, TAP_PROCESSED
    w, h = size
    what = "%s %dx%d balance %g: " % (name, w, h, balance)
    frame = bayer_frame(size)
    pipe = new_pipe()
    # debayer + undistortion only: the chain runs inside the remap's tiles; flips 0 / 180, footprint walk on
    pipe.set_taps(TAP_PROCESSED)
    pipe.set_tunable("chain_footprint", 1)
    for angle in (0, 180):
        c = cfg(flip=True, flip_angle=angle, undistort=True)
        cam, model, mx, my = setup(pipe, c, name, size, balance)
        got = pipe.process(frame, "bayer_rggb8")
        ref, enc = expected(oracle, c, frame, "bayer_rggb8", mx, my)
        assert enc == "bgr8" and pipe.last_encoding == "bgr8"
        assert_images_equal(got, ref, what + "debayer + undistortion, flip %d" % angle)
        assert ref.any(), what + "the expectation is black"
    # vignetting in front of the remap: two kernels, the chain walks the remap's footprint; then with all three taps
    c = cfg(flip=True, flip_angle=180, wb=True, wb_method="grey_world", cc=True, gamma=True, gamma_k=0.8, vig=True, undistort=True)
    setup(pipe, c, name, size, balance)
    ref, _, t_deb, t_col = expected(oracle, c, frame, "bayer_rggb8", mx, my, taps=True)
    assert_images_equal(pipe.process(frame, "bayer_rggb8"), ref, what + "two kernels, footprint walk")
    pipe.set_taps(TAP_PROCESSED | TAP_DEBAYERED | TAP_COLOR)
    assert_images_equal(pipe.process(frame, "bayer_rggb8"), ref, what + "two kernels, taps")
    assert_images_equal(pipe.get_dist_debayered_image(), t_deb.reshape(h, w, 3), what + "debayered tap")
    assert_images_equal(pipe.get_dist_color_image(), t_col.reshape(h, w, 3), what + "colour tap")
    assert_images_equal(pipe.get_processed_image(), ref, what + "processed tap")
    # mono8: the ring kernel gathers from the caller's frame
    mono = np.random.default_rng(w + h).integers(0, 256, (h, w), dtype=np.uint8)
    c = cfg(flip=True, flip_angle=180, gamma=True, gamma_k=0.8, undistort=True)
    setup(pipe, c, name, size, balance)
    ref, enc = expected(oracle, c, mono, "mono8", mx, my)
    got = pipe.process(mono, "mono8")
    assert enc == pipe.last_encoding
    assert_images_equal(got, ref, what + "mono8")
    # bgr8, undistortion only
    bgr = synth.gen_scene_bgr(w, h, seed=5)
    c = cfg(undistort=True)
    setup(pipe, c, name, size, balance)
    ref, enc = expected(oracle, c, bgr, "bgr8", mx, my)
    assert_images_equal(pipe.process(bgr, "bgr8"), ref, what + "bgr8")


PLUMB_BOB_CASE = ("barrel+k3", (200, 136), 1.0)


def test_mht_under_plumb_bob(oracle):
    from mht_reference import mht_reference
    name, size, balance = PLUMB_BOB_CASE
    frame = bayer_frame(size)
    pipe = new_pipe()
    c = cfg(flip=True, flip_angle=180, gamma=True, undistort=True)
    cam, model, mx, my = setup(pipe, c, name, size, balance)
    pipe.set_debayer_method("mht")
    ref, _ = expected(oracle, c, mht_reference(frame, "bayer_rggb8"), "bgr8", mx, my)
    assert_images_equal(pipe.process(frame, "bayer_rggb8"), ref, "mht")


def test_16_bit_frames_with_a_range_under_plumb_bob(oracle):
    import raw16_cases as G
    from raw16_reference import demosaic16, narrow16
    name, size, balance = PLUMB_BOB_CASE
    black, white = 256, 4095
    frame = G.gen_frame16(size[0], size[1], "rggb", 7, black, white)
    pipe = new_pipe()
    c = cfg(flip=True, flip_angle=180, wb=True, wb_method="grey_world", gamma=True, undistort=True)
    cam, model, mx, my = setup(pipe, c, name, size, balance)
    pipe.set_debayer_16bit(True)
    pipe.set_debayer_16bit_range(black, white)
    ref, _ = expected(oracle, c, narrow16(demosaic16(oracle, frame, "rggb", "bilinear"), black, white), "bgr8", mx, my)
    got = pipe.process(frame, "bayer_rggb16")
    assert pipe.last_encoding == "bgr8"
    assert_images_equal(got, ref, "bayer_rggb16 (%d, %d)" % (black, white))


def test_packed_12_bit_frames_under_plumb_bob(oracle):
    import packed_cases as PC
    import packed_reference as R
    from raw16_reference import demosaic16, narrow16
    name, size, balance = PLUMB_BOB_CASE
    black, white = 256, 4095
    samples = PC.gen_samples(size[0], size[1], "rggb", 9, "12p", black, white)
    pipe = new_pipe()
    c = cfg(gamma=True, undistort=True)
    cam, model, mx, my = setup(pipe, c, name, size, balance)
    pipe.set_debayer_16bit_range(black, white)
    ref, _ = expected(oracle, c, narrow16(demosaic16(oracle, samples, "rggb", "bilinear"), black, white), "bgr8", mx, my)
    assert_images_equal(pipe.process(R.pack(samples, "12p"), "bayer_rggb12p"), ref, "bayer_rggb12p")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_resident_batch_of_five(oracle, layout):
    import torch
    name, size, balance = "rational", (200, 136), 1.0
    w, h = size
    n = 5
    frames = np.stack([synth.gen_frame(w, h, "bayer_rggb8", seed=70 + i, kind="scene" if i % 2 == 0 else "uniform") for i in range(n)])
    pipe = new_pipe()
    c = cfg(flip=True, flip_angle=180, wb=True, wb_method="grey_world", cc=True, gamma=True, vig=True, undistort=True)
    cam, model, mx, my = setup(pipe, c, name, size, balance)
    batch = device_batch(frames, layout, np.random.default_rng(LAYOUTS.index(layout)))
    out = pipe.apply_device(batch.view, "bayer_rggb8")
    torch.cuda.synchronize()
    batch.check_padding("pinhole batch")
    out = out.cpu().numpy()
    for i in range(n):
        ref, _ = expected(oracle, c, frames[i], "bayer_rggb8", mx, my)
        assert_images_equal(out[i], ref, "%s frame %d" % (layout, i))


def test_switching_between_equidistant_and_plumb_bob_on_one_handle(oracle):
    """Each frame equals the expectation of the model that is set at that moment: a map or plan left over from the other
    model shows."""
    size, balance = (200, 136), 0.0
    frame = bayer_frame(size)
    pipe = new_pipe()
    fish = synth.camera_model(*size)
    c_fish = cfg(flip=True, flip_angle=180, vig=True, undistort=True, cam=fish, balance=balance)
    c_pin = dict(c_fish, cam=None)
    configure(pipe, c_fish)
    ref_fish, _ = oracle_run(oracle, c_fish, frame, "bayer_rggb8")
    cam, model, mx, my = reference("barrel+k3", size, balance)
    ref_pin, _ = expected(oracle, c_pin, frame, "bayer_rggb8", mx, my)
    assert not np.array_equal(ref_fish, ref_pin)
    assert_images_equal(pipe.process(frame, "bayer_rggb8"), ref_fish, "equidistant, first")
    for turn in range(2):
        pipe.set_undistortion_distortion_model(model)
        pipe.set_undistortion_camera_matrix(cam["K"])
        pipe.set_undistortion_distortion_coeffs(cam["D"])
        assert pipe.get_dist_distortion_coefficients().shape == (1, 5)
        assert_images_equal(pipe.process(frame, "bayer_rggb8"), ref_pin, "plumb_bob, turn %d" % turn)
        pipe.set_undistortion_distortion_coeffs(fish["D"])
        pipe.set_undistortion_camera_matrix(fish["K"])
        pipe.set_undistortion_distortion_model("equidistant")
        assert pipe.get_dist_distortion_coefficients().shape == (1, 4)
        assert_images_equal(pipe.process(frame, "bayer_rggb8"), ref_fish, "equidistant, turn %d" % turn)
