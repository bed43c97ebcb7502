"""Every kernel instantiation of the library ran, and equals the oracle (tests/variant_cases.py; PARITY.md "Variant coverage").

One test per launch record.  Each configures a fresh handle through the public setters with the launch log on, runs the case as
a resident batch of different frames (scene, uniform noise, tinted scene, ...) so that the frame loop and the per-frame
statistics are live, asserts that the expected record is in the log -- and, where a fast variant is expected, that no generic
kernel is -- and compares every frame with the CPU oracle at tolerance 0, under the oracle's contracted model for the fc=1 twins."""
import functools

import numpy as np
import pytest

import packed_cases as PC
import packed_reference as R
import pinhole_reference as PR
import raw16_cases as G
import variant_cases as V
from helpers import assert_images_equal, cfg, configure, oracle_params, oracle_run
from mht_reference import flip as np_flip, mht_reference
from raw16_reference import demosaic16, narrow16
from raw_image_pipeline_amd import TAP_PROCESSED, RawImagePipeline, synth

pytestmark = pytest.mark.gpu

TINTS = [(0.70, 1.00, 0.55), (1.0, 1.0, 1.0), (0.55, 1.00, 0.80), (0.9, 1.0, 0.6)]


def kind_of(i):
    return "uniform" if i % 3 == 1 else "scene"


@functools.lru_cache(maxsize=None)
def frames_of(source, pattern, w, h, n, layout, range16):
    """The n different frames of a case as the oracle's side sees them: uint8 Bayer / BGR / mono, or uint16 samples.  Frame 1 is
    uniform noise, the others scenes under different tints.  Shared between the cases; read-only."""
    out = []
    for i in range(n):
        tint, seed = TINTS[i % len(TINTS)], 40 + i
        if source == "bayer8":
            f = synth.gen_frame(w, h, "bayer_%s8" % pattern, seed=seed, kind=kind_of(i), tint=tint)
        elif source == "mono8":
            f = synth.gen_frame(w, h, "bayer_rggb8", seed=seed, kind=kind_of(i), tint=tint)
        elif source == "bgr8":
            f = synth.gen_scene_bgr(w, h, seed, tint) if kind_of(i) == "scene" else np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
        elif source == "bayer16":
            f = G.gen_frame16(w, h, pattern, seed, 0, 65535, kind="random" if kind_of(i) == "uniform" else "scene", tint=tint)
        elif source == "raw16":
            f = G.gen_frame16(w, h, pattern, seed, range16[0], range16[1], kind="random" if kind_of(i) == "uniform" else "scene", tint=tint)
        else:
            assert source == "packed", source
            f = PC.gen_samples(w, h, pattern, seed, layout, range16[0], range16[1], kind="random" if kind_of(i) == "uniform" else "scene", tint=tint)
        f.setflags(write=False)
        out.append(f)
    assert len({f.tobytes() for f in out}) == n
    return out


def encoding_of(case):
    if case.source == "bayer8":
        return "bayer_%s8" % case.pattern
    if case.source in ("bayer16", "raw16"):
        return G.enc16(case.pattern)
    if case.source == "packed":
        return R.enc(case.pattern, case.layout)
    return case.source


def device_form(case, frame):
    """The bytes the library is given for a frame."""
    if case.source in ("bayer16", "raw16"):
        f = np.ascontiguousarray(frame, np.uint16)
        return f.view(np.uint8).reshape(f.shape[0], f.shape[1] * 2)
    if case.source == "packed":
        return R.pack(frame, case.layout)
    return frame


@functools.lru_cache(maxsize=None)
def pinhole_maps(camera, size, balance, fov_scale):
    """The maps of a pinhole camera from tests/pinhole_reference.py alone.  Shared; read-only."""
    _, model, D, new_size = camera
    cam = synth.pinhole_camera_model(size[0], size[1], D)
    newK = PR.new_camera_matrix(cam["K"], model, list(D), size, balance, new_size, fov_scale)
    mx, my = PR.maps(cam["K"], model, list(D), cam["R"], newK, size)
    return np.ascontiguousarray(mx), np.ascontiguousarray(my)


def setup(pipe, case, c, size):
    configure(pipe, c)
    if isinstance(case.camera, tuple):
        _, model, D, new_size = case.camera
        synth.load_camera(pipe, synth.pinhole_camera_model(size[0], size[1], D), model)
        pipe.set_undistortion_balance(c["balance"])
        pipe.set_undistortion_fov_scale(c["fov_scale"])
        if new_size:
            pipe.set_undistortion_new_image_size(*new_size)
    pipe.set_debayer_method(case.method)
    pipe.set_debayer_16bit(case.source in ("bayer16", "raw16"))
    pipe.set_debayer_16bit_range(*(case.range16 or (0, 0)))
    for name, value in case.tunables.items():
        pipe.set_tunable(name, value)
    pipe.set_fp_contraction(case.fc)


def expectation(O, case, c, size, frame, occ):
    """The oracle's image of one frame.  MHT, 16-bit and packed frames are processed like the bgr8 frame holding their demosaiced
    (and narrowed) image, as tests/test_debayer_mht_gpu.py, test_raw16_gpu.py and test_packed_gpu.py build their expectations."""
    enc = encoding_of(case)
    if case.source == "bayer16":   # debayer + flip only, 16 bits out
        img = demosaic16(O, frame, case.pattern, case.method)
        return np_flip(img, c["flip_angle"] if c["flip"] else 0)
    if case.source in ("raw16", "packed"):
        frame, enc = narrow16(demosaic16(O, frame, case.pattern, case.method), *case.range16), "bgr8"
    elif case.source == "bayer8" and case.method == "mht":
        frame, enc = mht_reference(frame, enc), "bgr8"
    with O.fp_contraction(case.fc):
        if isinstance(case.camera, tuple):
            mx, my = pinhole_maps(case.camera, size, c["balance"], c["fov_scale"])
            keep = []
            prm = oracle_params(O, c, keep)
            prm.und_enabled = 1
            prm.map_x, prm.map_y = mx.ctypes.data, my.ctypes.data
            prm.map_rows, prm.map_cols = mx.shape
            return O.pipeline(prm, np.ascontiguousarray(frame), enc, ccc=occ)[0]
        return oracle_run(O, c, np.ascontiguousarray(frame), enc, ccc=occ)[0]


def ccc_pair(pipe, O, c):
    if not (c["wb"] and c["wb_method"] == "ccc"):
        return None
    filt, bias = synth.ccc_model()
    pipe.set_ccc_model(filt, bias)
    return O.CCC(filt, bias)


def check_log(case, log, what):
    keys = log.keys()
    assert (case.name, case.fc) in keys, "%s: no launch of %s fc=%d; the log holds\n%s" % (what, case.name, case.fc, log.text)
    if case.fast:
        generic = sorted(V.GENERIC_KERNELS & {k for k, _ in keys})
        assert not generic, "%s: a fast variant was expected, the log holds %s" % (what, generic)
    for r in log.records():
        assert r["grid"][0] >= 1 and r["grid"][1] >= 1 and r["block"] in (64, 256, 512, 1024), r


def run_size(O, case, size):
    import torch
    w, h = size
    cam = synth.camera_model(w, h) if case.camera == "fisheye" else None
    c = cfg(cam=cam, **case.cfg)
    what = "%s %dx%d" % (V.case_id(case), w, h)
    frames = frames_of(case.source, case.pattern, w, h, case.n_frames, case.layout, case.range16)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    enc = encoding_of(case)
    kw = dict(width=w) if case.source == "packed" else {}
    with pipe.launch_log() as log:   # on before the configuration: the maps and tables a frame builds lazily are launches too
        setup(pipe, case, c, size)
        occ = ccc_pair(pipe, O, c)
        batch = torch.from_numpy(np.stack([device_form(case, f) for f in frames])).cuda()
        out = pipe.apply_device(batch, enc, **kw)
        torch.cuda.synchronize()
    check_log(case, log, what)
    out = out.cpu().numpy()
    if case.source == "bayer16":
        out = out.view(np.uint16).reshape(out.shape[0], out.shape[1], out.shape[2], 3)
    refs = []
    for i, f in enumerate(frames):
        ref = expectation(O, case, c, size, f, occ)
        assert ref.min() != ref.max(), what + ": the expectation of frame %d is a constant image" % i
        got = out[i].reshape(ref.shape)
        if ref.dtype == np.uint16:
            assert np.array_equal(got, ref), "%s frame %d: max |diff| %d" % (what, i, int(np.abs(got.astype(np.int64) - ref).max()))
        else:
            assert_images_equal(got, ref, "%s frame %d/%d" % (what, i, len(frames)))
        refs.append(ref)
    if case.single_frame:   # the same variant from one process() call: the launch geometry of one or two frames
        pipe.set_taps(TAP_PROCESSED)
        occ = ccc_pair(pipe, O, c)
        with pipe.launch_log() as log:
            got = pipe.process(device_form(case, frames[0]), enc, **kw)
        check_log(case, log, what + " single frame")
        assert all(r["frames"] in (0, 1) for r in log.records()), log.text
        assert_images_equal(got.reshape(refs[0].shape), refs[0], what + " single frame")


@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_variant_ran_and_equals_the_oracle(rip_lib, oracle, case):
    for size in case.sizes:
        run_size(oracle, case, size)
