"""The constants a handle keeps on the device -- colour tables, vignetting mask, undistortion maps with their remap plan and
item list, the ccc estimator's resize geometry, the output table and the resize tables -- when a setting changes on a LIVE
handle between frames.  Most other tests start from a fresh handle, so the code that notices a change and uploads the constant
again is what runs here: one handle per test, every step against the reference at tolerance 0."""
import numpy as np
import pytest

import area_reference as A
import output_reference as R
import wb_degenerate_cases as D
from helpers import assert_images_equal, cfg, configure, oracle_run
from raw_image_pipeline_amd import RawImagePipeline, synth
from test_chain_footprint_gpu import chain_cfg, frames_on_device, new_pipe
from test_output_format_gpu import NORM, delivered
from test_resize_gpu import noise, resized, trusted

pytestmark = pytest.mark.gpu


def step(pipe, O, c, frame, encoding, what, ccc=None, fp_contract=0):
    """One frame through the handle AS IT STANDS (no configure: that would mark every constant dirty) against the oracle under c."""
    got = pipe.process(frame, encoding)
    with O.fp_contraction(fp_contract):
        ref, enc = oracle_run(O, c, frame, encoding, ccc=ccc)
    assert pipe.last_encoding == enc
    assert_images_equal(got, ref, what)


def test_colour_tables_follow_the_gamma_settings(gpu_pipe, oracle):
    w, h = 64, 48
    frame = synth.gen_frame(w, h, "bayer_rggb8", seed=61, kind="scene")
    c = cfg(gamma=True, gamma_k=0.8, cc=True)
    configure(gpu_pipe, c)
    step(gpu_pipe, oracle, c, frame, "bayer_rggb8", "gamma k 0.8")
    step(gpu_pipe, oracle, c, frame, "bayer_rggb8", "gamma k 0.8, nothing changed")
    c = dict(c, gamma_k=2.2)
    gpu_pipe.set_gamma_correction_k(2.2)
    step(gpu_pipe, oracle, c, frame, "bayer_rggb8", "gamma k 2.2")
    c = dict(c, gamma=False)
    gpu_pipe.set_gamma_correction(False)
    step(gpu_pipe, oracle, c, frame, "bayer_rggb8", "gamma off")
    c = dict(c, gamma=True)
    gpu_pipe.set_gamma_correction(True)
    step(gpu_pipe, oracle, c, frame, "bayer_rggb8", "gamma on again, k 2.2")


def test_vignetting_mask_follows_parameters_geometry_and_contraction_model(gpu_pipe, oracle):
    wide = synth.gen_frame(64, 48, "bayer_rggb8", seed=62, kind="uniform")
    tall = synth.gen_frame(48, 64, "bayer_rggb8", seed=63, kind="uniform")
    c = cfg(vig=True, gamma=True, flip=True, flip_angle=180)
    configure(gpu_pipe, c)
    step(gpu_pipe, oracle, c, wide, "bayer_rggb8", "vignetting 64x48")
    c = dict(c, vig_params=(1.2, 2e-3, 3e-6))
    gpu_pipe.set_vignetting_correction_parameters(*c["vig_params"])
    step(gpu_pipe, oracle, c, wide, "bayer_rggb8", "vignetting 64x48, other parameters")
    # the mask is keyed by geometry: no setter is called between these three
    step(gpu_pipe, oracle, c, tall, "bayer_rggb8", "vignetting 48x64")
    step(gpu_pipe, oracle, c, wide, "bayer_rggb8", "vignetting 64x48 again")
    step(gpu_pipe, oracle, c, wide, "bayer_rggb8", "vignetting 64x48, nothing changed")
    for mode in (0, 1, 0):
        gpu_pipe.set_fp_contraction(mode)
        step(gpu_pipe, oracle, c, wide, "bayer_rggb8", "vignetting 64x48, contraction model %d" % mode, fp_contract=mode)
        step(gpu_pipe, oracle, c, tall, "bayer_rggb8", "vignetting 48x64, contraction model %d" % mode, fp_contract=mode)


def test_maps_plan_and_item_list_follow_calibration_flip_and_camera(oracle):
    """328 x 200: the smallest geometry of test_chain_footprint_gpu.py whose footprint is smaller than the frame."""
    import torch
    n = 3
    pipe = new_pipe()
    pipe.set_tunable("chain_footprint", 1)
    batches = {size: frames_on_device(size[0], size[1], n, seed=70) for size in ((328, 200), (320, 240))}

    def batch(c, what, footprint):
        w, h = c["cam"]["width"], c["cam"]["height"]
        frames = batches[(w, h)]
        out = pipe.apply_device(frames, "bayer_rggb8")
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        for k in range(n):
            ref, _ = oracle_run(oracle, c, frames[k].cpu().numpy(), "bayer_rggb8")
            assert_images_equal(out[k], ref, "%s, frame %d" % (what, k))
        fp, _ = pipe.debug_chain_footprint(h, w, c["flip_angle"])
        if footprint:
            assert fp["last_walked"] == fp["footprint_items"] < fp["dense_items"], (what, fp)
        else:
            assert fp["last_walked"] in (fp["footprint_items"], fp["dense_items"]), (what, fp)
        info = pipe.debug_plan_info(h, w)
        assert info["tiles_x"] == -(-w // info["tile_w"]) and info["tiles_y"] == -(-h // info["tile_h"]) and info["on_device"] == 1, (what, info)

    c = chain_cfg(328, 200, flip_angle=0)
    configure(pipe, c)
    batch(c, "328x200", True)
    batch(c, "328x200, nothing changed", True)
    for balance in (1.0, 0.0):
        c = dict(c, balance=balance)
        pipe.set_undistortion_balance(balance)
        batch(c, "balance %g" % balance, balance == 0.0)
    for fov in (0.8, 1.0):
        c = dict(c, fov_scale=fov)
        pipe.set_undistortion_fov_scale(fov)
        batch(c, "fov_scale %g" % fov, fov == 1.0)
    for angle in (180, 0):  # the calibration untouched: the plan stays, the item list is per (plan, flip)
        c = dict(c, flip_angle=angle)
        pipe.set_flip_angle(angle)
        batch(c, "flip %d" % angle, True)
    other = chain_cfg(320, 240, flip_angle=0)
    configure(pipe, other)
    batch(other, "a camera of 320x240", True)
    configure(pipe, c)
    batch(c, "the camera of 328x200 again", True)


def test_ccc_geometry_follows_the_frame_size(gpu_pipe, oracle):
    """The estimator's 360 x 270 resize tables are keyed by the frame's size; 720 x 540 is the exact 2 x 2 case."""
    gpu_pipe.load_ccc_model(D.default_model_path())
    gpu_pipe.set_ccc_kalman_model(1.0, 10.0)
    occ = oracle.CCC(*D.load_default_model())
    occ.set_kalman_model(1.0, 10.0)
    c = cfg(wb=True, wb_method="ccc", wb_bright=0.8, wb_dark=0.2, wb_temporal=False)
    configure(gpu_pipe, c)
    for k, (w, h) in enumerate(((384, 240), (720, 540), (250, 190), (720, 540))):
        frame = synth.gen_frame(w, h, "bayer_gbrg8", seed=7100 + k, kind="scene", tint=(0.62 + 0.05 * k, 1.0, 0.5))
        step(gpu_pipe, oracle, c, frame, "bayer_gbrg8", "ccc %dx%d (step %d)" % (w, h, k), ccc=occ)
        gpu_pipe.reset_white_balance_temporal_consistency()
        occ.reset()


def test_output_table_and_resize_tables_follow_their_settings(rip_lib, oracle):
    import torch
    w, h, n = 64, 48, 2
    e = trusted(w, h, n, 3)
    frames = torch.from_numpy(noise(w, h, n, 3).copy()).cuda()
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, cfg())

    def batch(fmt, norm, target, interpolation, what):
        out = pipe.apply_device(frames, "bgr8")
        torch.cuda.synchronize()
        r = e
        if target is not None:
            r = A.resize_stack(e, target[1], target[0]) if interpolation == "area" else resized(oracle, e, target[1], target[0])
        ref = R.convert(r, fmt, *norm)
        assert tuple(out.shape) == ref.shape, (what, out.shape, ref.shape)
        got = delivered(out)
        assert np.array_equal(got, R.bits(ref)), "%s: %d of %d elements differ" % (what, int((got != R.bits(ref)).sum()), got.size)

    other_norm = (128.0, (0.25, 0.5, 0.75), (0.5, 2.0, 1.5))
    pipe.set_output_format("rgb_chw_f32")
    pipe.set_output_normalization(*NORM)
    batch("rgb_chw_f32", NORM, None, None, "f32")
    pipe.set_output_normalization(*other_norm)
    batch("rgb_chw_f32", other_norm, None, None, "f32, other normalisation")
    batch("rgb_chw_f32", other_norm, None, None, "f32, nothing changed")
    pipe.set_output_format("rgb_chw_f16")
    batch("rgb_chw_f16", other_norm, None, None, "f16")
    pipe.set_output_format("rgb_chw_f32")
    batch("rgb_chw_f32", other_norm, None, None, "f32 again")
    # the linear and the area tables share one buffer and one key
    for target, interpolation in (((32, 24), "linear"), ((40, 30), "linear"), ((16, 12), "area"), ((21, 17), "area"), ((40, 30), "linear")):
        pipe.set_output_interpolation(interpolation)
        pipe.set_output_size(*target)
        batch("rgb_chw_f32", other_norm, target, interpolation, "%s to %dx%d" % ((interpolation,) + target))
        batch("rgb_chw_f32", other_norm, target, interpolation, "%s to %dx%d, nothing changed" % ((interpolation,) + target))
