"""The fused Bayer chain in front of the remap walks only the remap's footprint (ChainParams::item_list, tunable
chain_footprint): outputs must be byte-identical to the dense walk and to the oracle, with the skipped pixels of the
intermediate image holding stale data of another stage set; the footprint the device compiles must equal the host's; a tap
must bring the dense walk back.  rip_debug_chain_footprint's last_walked tells which walk ran."""
import numpy as np
import pytest

from helpers import assert_images_equal, cfg, configure, oracle_run
from raw_image_pipeline_amd import synth

pytestmark = pytest.mark.gpu


def chain_cfg(w, h, flip_angle=180, **kw):
    base = dict(flip=True, flip_angle=flip_angle, wb=True, wb_method="grey_world", cc=True, gamma=True, gamma_k=0.8, vig=True,
                undistort=True, cam=synth.camera_model(w, h))
    base.update(kw)
    return cfg(**base)


def new_pipe():
    from raw_image_pipeline_amd import RawImagePipeline, TAP_PROCESSED
    p = RawImagePipeline(False, "", "", "", device=0)
    p.set_taps(TAP_PROCESSED)  # no debayered / colour tap: the chain writes the internal intermediate image
    return p


def frames_on_device(w, h, n, seed):
    import torch
    base = [synth.gen_frame(w, h, "bayer_rggb8", seed=seed + k, kind="scene") for k in range(min(n, 4))]
    t = torch.from_numpy(np.stack([base[k % len(base)] for k in range(n)])).cuda()
    if n > len(base):  # distinct frames for the per-frame grey-world gains
        t[len(base):] = torch.roll(t[len(base):], shifts=1, dims=0) // 2 + 17
    return t


def poison(pipe, c, frames):
    """Run another stage set (enhancer instead of vignetting, other gains) densely on the same handle: the intermediate image
    then holds other values everywhere, also where the footprint walk will not write."""
    pipe.set_tunable("chain_footprint", 0)
    configure(pipe, dict(c, vig=False, ce=True, ce_sat=1.3, cc_bias=(0.0, 0.0, 0.0), gamma_k=0.6))
    pipe.apply_device(frames, "bayer_rggb8")
    configure(pipe, c)


@pytest.mark.parametrize("fp_contract", [0, 1])
@pytest.mark.parametrize("flip_angle", [0, 180])
@pytest.mark.parametrize("size,n", [((2448, 2048), 1), ((2448, 2048), 3), ((640, 480), 256), ((328, 200), 3)])
def test_footprint_walk_equals_dense_walk(oracle, size, n, flip_angle, fp_contract):
    import torch
    w, h = size
    c = chain_cfg(w, h, flip_angle=flip_angle)
    frames = frames_on_device(w, h, n, seed=40 + n)
    pipe = new_pipe()
    pipe.set_fp_contraction(fp_contract)
    configure(pipe, c)
    poison(pipe, c, frames)
    pipe.set_tunable("chain_footprint", 1)
    got = pipe.apply_device(frames, "bayer_rggb8")
    torch.cuda.synchronize()
    info, _ = pipe.debug_chain_footprint(h, w, flip_angle)
    assert info["last_walked"] == info["footprint_items"] < 0.95 * info["dense_items"], info
    pipe.set_tunable("chain_footprint", 0)
    dense = pipe.apply_device(frames, "bayer_rggb8")
    torch.cuda.synchronize()
    assert pipe.debug_chain_footprint(h, w, flip_angle)[0]["last_walked"] == info["dense_items"]
    assert torch.equal(got, dense), "footprint walk differs from the dense walk on %d bytes" % int((got != dense).sum())
    if fp_contract == 0:
        for k in sorted({0, n - 1}):
            ref, _ = oracle_run(oracle, c, frames[k].cpu().numpy(), "bayer_rggb8")
            assert_images_equal(got[k].cpu().numpy(), ref, "frame %d vs oracle" % k)


def test_config2_batch_of_256_bit_identical(oracle):
    """The benchmark's batch: 256 frames of 2448 x 2048 through vignetting + undistortion, footprint on and off."""
    import torch
    w, h, n = 2448, 2048, 256
    c = chain_cfg(w, h)
    frames = frames_on_device(w, h, n, seed=3)
    pipe = new_pipe()
    configure(pipe, c)
    poison(pipe, c, frames)
    pipe.set_tunable("chain_footprint", 1)
    got = pipe.apply_device(frames, "bayer_rggb8")
    torch.cuda.synchronize()
    info, _ = pipe.debug_chain_footprint(h, w, 180)
    assert info["last_walked"] == info["footprint_items"]
    assert abs(info["footprint_items"] / info["dense_items"] - 0.785) <= 0.01
    pipe.set_tunable("chain_footprint", 0)
    dense = pipe.apply_device(frames, "bayer_rggb8")
    torch.cuda.synchronize()
    assert torch.equal(got, dense)
    del dense
    ref, _ = oracle_run(oracle, c, frames[n - 1].cpu().numpy(), "bayer_rggb8")
    assert_images_equal(got[n - 1].cpu().numpy(), ref, "last frame vs oracle")


@pytest.mark.parametrize("flip_angle", [0, 180])
def test_vignetting_enhancer_undistortion_small(oracle, flip_angle):
    w, h = 320, 240
    c = chain_cfg(w, h, flip_angle=flip_angle, ce=True, ce_sat=1.2, ce_val=0.9)
    frame = synth.gen_frame(w, h, "bayer_rggb8", seed=9, kind="scene")
    pipe = new_pipe()
    configure(pipe, c)
    poison(pipe, c, frames_on_device(w, h, 1, seed=9))
    pipe.set_tunable("chain_footprint", 1)
    got = pipe.process(frame, "bayer_rggb8")
    info, _ = pipe.debug_chain_footprint(h, w, flip_angle)
    assert info["last_walked"] == info["footprint_items"] < info["dense_items"]
    ref, _ = oracle_run(oracle, c, frame, "bayer_rggb8")
    assert_images_equal(got, ref, "vignetting + enhancer + undistortion, flip %d" % flip_angle)


@pytest.mark.parametrize("size,balance,fov,shift", [((2448, 2048), 0.0, 1.0, False), ((3840, 2160), 0.0, 1.0, False),
                                                    ((640, 480), 0.5, 1.0, False), ((640, 480), 1.0, 1.0, False),
                                                    ((648, 484), 0.0, 0.6, True), ((648, 484), 0.0, 1.4, False)])
def test_footprint_compiled_on_the_device_equals_the_host_footprint(rip_lib, monkeypatch, size, balance, fov, shift):
    from raw_image_pipeline_amd import RawImagePipeline
    w, h = size
    cam = synth.camera_model(w, h)
    if shift:
        K = list(cam["K"])
        K[2] += 0.07 * w
        K[5] -= 0.05 * h
        cam["K"] = K
    c = cfg(undistort=True, cam=cam, balance=balance, fov_scale=fov)
    dev = RawImagePipeline(False, "", "", "", device=0)
    configure(dev, c)
    monkeypatch.setenv("RIP_PLAN_ON_HOST", "1")
    host_plan = RawImagePipeline(False, "", "", "", device=0)
    configure(host_plan, c)
    monkeypatch.delenv("RIP_PLAN_ON_HOST")
    cpu = RawImagePipeline(False, "", "", "", device=-1)
    configure(cpu, c)
    assert dev.debug_plan_info(h, w)["on_device"] == 1 and host_plan.debug_plan_info(h, w)["on_device"] == 0
    for flip in (0, 180):
        i_d, iv_d = dev.debug_chain_footprint(h, w, flip)
        i_h, iv_h = host_plan.debug_chain_footprint(h, w, flip)
        i_c, iv_c = cpu.debug_chain_footprint(h, w, flip)
        assert np.array_equal(iv_d, iv_h) and np.array_equal(iv_d, iv_c), (size, balance, fov, flip)
        assert i_d["footprint_items"] == i_h["footprint_items"] == i_c["footprint_items"]


@pytest.mark.parametrize("which", ["debayered", "color"])
def test_a_tap_brings_the_dense_walk_back(oracle, which):
    import torch
    from raw_image_pipeline_amd import TAP_COLOR, TAP_DEBAYERED, TAP_PROCESSED
    w, h = 640, 480
    c = chain_cfg(w, h)
    frame = synth.gen_frame(w, h, "bayer_rggb8", seed=12, kind="scene")
    pipe = new_pipe()
    configure(pipe, c)
    poison(pipe, c, frames_on_device(w, h, 1, seed=12))
    pipe.set_tunable("chain_footprint", 1)
    pipe.set_taps(TAP_PROCESSED | (TAP_DEBAYERED if which == "debayered" else TAP_COLOR))
    got = pipe.process(frame, "bayer_rggb8")
    info, _ = pipe.debug_chain_footprint(h, w, 180)
    assert info["last_walked"] == info["dense_items"] > info["footprint_items"]
    ref, _, t_deb, t_col = oracle_run(oracle, c, frame, "bayer_rggb8", taps=True)
    assert_images_equal(got, ref, "final")
    if which == "debayered":
        assert_images_equal(pipe.get_dist_debayered_image(), t_deb.reshape(h, w, 3), "debayered tap")
    else:
        assert_images_equal(pipe.get_dist_color_image(), t_col.reshape(h, w, 3), "colour tap")
    # the same through the device entry point with a caller-owned colour tap
    t = torch.from_numpy(frame[None]).cuda()
    tap = torch.empty((1, h, w, 3), dtype=torch.uint8, device="cuda")
    out = pipe.apply_device(t, "bayer_rggb8", tap_color=tap)
    torch.cuda.synchronize()
    assert pipe.debug_chain_footprint(h, w, 180)[0]["last_walked"] == info["dense_items"]
    assert_images_equal(tap[0].cpu().numpy(), t_col.reshape(h, w, 3), "caller's colour tap")
    assert_images_equal(out[0].cpu().numpy(), ref, "final (device entry point)")
