"""White balance on degenerate frames and with the reference's own ccc model, against the CPU oracle at tolerance 0
(tests/wb_degenerate_cases.py; PARITY.md "Degenerate frames").

What is compared: the image of every frame, and every estimate the library exposes -- grey-world's Q8 gains, SimpleWB's alpha, the
ccc gains, (u, v) and track -- field by field, NaN equal to NaN and otherwise equal float32 bits.  The launch log says which
statistics kernel produced them."""
import functools

import numpy as np
import pytest

import wb_degenerate_cases as D
from helpers import assert_images_equal, assert_launched, cfg, configure
from raw_image_pipeline_amd import synth

pytestmark = pytest.mark.gpu

PCA_KERNEL, GREY_KERNEL, SIMPLE_KERNEL = "stats_fast_kernel<3>", "stats_fast_kernel<1>", "stats_fast_kernel<4>"   # rip::WbMode


def check_estimate(what, method, est, info, track):
    """The exposed estimate of one frame (a row of get_white_balance_info, a row of get_ccc_track) against the oracle's."""
    if method == "grey_world":
        assert [float(v) for v in info[3:6]] == [float(v) for v in est["q8"]], "%s: q8 %s, oracle %s" % (what, info[3:6], est["q8"])
    elif method == "simple":
        assert D.same_floats(info[0:3], est["ab"][0::2]), "%s: alpha %s, oracle %s" % (what, info[0:3], est["ab"][0::2])
    elif method == "ccc":
        assert [int(v) for v in track] == est["track"], "%s: track %s, oracle %s" % (what, track, est["track"])
        assert [int(v) for v in info[6:8]] == est["track"][2:4], what
        assert D.same_floats(info[0:3], est["gains"]), "%s: gains %s, oracle %s" % (what, info[0:3], est["gains"])


def set_model(pipe, O, model):
    """The ccc model on the handle and an oracle object built from the same bytes."""
    if model == "default":
        pipe.load_ccc_model(D.default_model_path())
    else:
        pipe.set_ccc_model(*D.model_arrays(model))
    pipe.set_ccc_kalman_model(1.0, 10.0)
    occ = O.CCC(*D.model_arrays(model))
    occ.set_kalman_model(1.0, 10.0)
    return occ


def run_frames(pipe, O, method, params, form, frames, occ, what, single=True, kernels=(), forbidden=()):
    """Every frame through process() (when `single`) and all of them as one resident batch through apply_device(): images and
    exposed estimates against the oracle's single-frame results."""
    import torch
    exps = []
    for f in frames:
        if occ is not None:
            occ.reset()
        exps.append(D.expected(O, method, params, form, f, occ))
    n = len(frames)
    if single:
        for i, f in enumerate(frames):
            with pipe.launch_log() as log:
                got = pipe.process(f, form)
            w = "%s frame %d, process" % (what, i)
            assert_launched(log, kernels, forbidden, w)
            assert_images_equal(got, exps[i].image, w)
            check_estimate(w, method, exps[i].estimate, pipe.get_white_balance_info(1)[0], pipe.get_ccc_track(1)[0])
    with pipe.launch_log() as log:
        out = pipe.apply_device(torch.from_numpy(np.stack(frames)).cuda(), form)
        torch.cuda.synchronize()
    assert_launched(log, kernels, forbidden, what + " batch")
    out = out.cpu().numpy()
    info, track = pipe.get_white_balance_info(n), pipe.get_ccc_track(n)
    for i in range(n):
        w = "%s frame %d of a batch of %d" % (what, i, n)
        assert_images_equal(out[i], exps[i].image, w)
        check_estimate(w, method, exps[i].estimate, info[i], track[i])
    return log


GROUPS = D.groups()


@pytest.mark.parametrize("key", list(GROUPS), ids=D.group_id)
def test_every_case_through_process_and_apply_device(gpu_pipe, oracle, key):
    """The twelve content kinds of one (setting, form, size): each as a single host frame and all twelve as one resident batch."""
    cases = GROUPS[key]
    c0 = cases[0]
    configure(gpu_pipe, cfg(wb=True, wb_method=c0.method, wb_temporal=False, **c0.params))
    occ = set_model(gpu_pipe, oracle, c0.model) if c0.method == "ccc" else None
    frames = [D.frame(c.kind, c.form, *c.size) for c in cases]
    if c0.method == "ccc":
        kernels, forbidden = ["ccc_hist*kernel", "wb_finalize_kernel"], ["stats_*"]   # twelve frames reach the LDS histogram
    else:
        kernels = [D.expected_stats_kernel(c0.form, c0.size)]
        forbidden = [k for k in ("stats_fast_kernel<?>", "stats_color_kernel", "stats_generic_kernel") if k != kernels[0]]
    run_frames(gpu_pipe, oracle, c0.method, c0.params, c0.form, frames, occ, D.group_id(key), kernels=kernels, forbidden=forbidden)


# ---- mixed batches: a frame whose workgroup totals are all zero skips its atomics, yet draws its ticket and hands its record back clean ----
def ordinary(form, w, h, seed):
    if form.startswith("bayer_"):
        return synth.gen_frame(w, h, form, seed=seed, kind="scene", tint=(0.6 + 0.02 * (seed % 10), 1.0, 0.55))
    return synth.gen_scene_bgr(w, h, seed, (0.6 + 0.02 * (seed % 10), 1.0, 0.55))


@pytest.mark.parametrize("form,size", [("bayer_rggb8", (64, 48)), ("bayer_gbrg8", (132, 36)), ("bgr8", (64, 48)), ("bgr8", (51, 33))],
                         ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
@pytest.mark.parametrize("method,params", [("grey_world", dict(wb_bright=0.8)), ("pca", {}), ("simple", dict(wb_percentile=10.0))],
                         ids=["grey_world", "pca", "simple"])
def test_mixed_batches_on_one_handle(gpu_pipe, oracle, method, params, form, size):
    w, h = size
    configure(gpu_pipe, cfg(wb=True, wb_method=method, **params))
    mixed = [ordinary(form, w, h, 910), D.frame("black", form, w, h), ordinary(form, w, h, 911), D.frame("white", form, w, h),
             D.frame("flat_colour", form, w, h), D.frame("blown", form, w, h), ordinary(form, w, h, 912)]
    what = "%s %s %dx%d" % (method, form, w, h)
    kernels = [D.expected_stats_kernel(form, size)]
    run_frames(gpu_pipe, oracle, method, params, form, mixed, None, what + " mixed", single=False, kernels=kernels)
    run_frames(gpu_pipe, oracle, method, params, form, [ordinary(form, w, h, 920 + i) for i in range(17)], None, what + " 17 ordinary",
               single=False, kernels=kernels)
    run_frames(gpu_pipe, oracle, method, params, form, mixed[::-1], None, what + " mixed again", single=False, kernels=kernels)


def test_ccc_track_alternating_between_the_sample_frame_and_a_black_one(gpu_pipe, oracle):
    """default.bin, temporal consistency on, Kalman model (1, 10): the raw arg-max jumps between the sample frame's (111, 139) and
    the bias peak (166, 106) of the empty histogram; the filtered track must equal the oracle's CCC object frame by frame, as one
    batch and as single calls carrying the filter state on."""
    import torch
    params = dict(wb_bright=0.8, wb_dark=0.2)
    configure(gpu_pipe, cfg(wb=True, wb_method="ccc", wb_temporal=True, **params))
    occ = set_model(gpu_pipe, oracle, "default")
    occ.set_temporal_consistency(True)
    gpu_pipe.reset_white_balance_temporal_consistency()
    sample = D.sample_image()
    frames = [sample if i % 2 == 0 else np.zeros_like(sample) for i in range(7)]
    exps = [D.expected(oracle, "ccc", params, "bgr8", f, occ) for f in frames + frames[:4]]
    assert [e.estimate["track"][0:2] for e in exps[:2]] == [[111, 139], [166, 106]]
    assert any(e.estimate["track"][0:2] != e.estimate["track"][2:4] for e in exps), "the filter must lag the jumps"
    out = gpu_pipe.apply_device(torch.from_numpy(np.stack(frames)).cuda(), "bgr8")
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    info, track = gpu_pipe.get_white_balance_info(7), gpu_pipe.get_ccc_track(7)
    for i in range(7):
        check_estimate("batch frame %d" % i, "ccc", exps[i].estimate, info[i], track[i])
        assert_images_equal(out[i], exps[i].image, "batch frame %d" % i)
    for i in range(4):
        got = gpu_pipe.process(frames[i], "bgr8")
        check_estimate("single call %d" % i, "ccc", exps[7 + i].estimate, gpu_pipe.get_white_balance_info(1)[0], gpu_pipe.get_ccc_track(1)[0])
        assert_images_equal(got, exps[7 + i].image, "single call %d" % i)


# ---- the statistics kernel at the edge of its 32-bit wave sums --------------------------------------------------------------
@pytest.mark.parametrize("method,params,kernel", [("pca", {}, PCA_KERNEL), ("grey_world", dict(wb_bright=1.0), GREY_KERNEL),
                                                  ("simple", dict(wb_percentile=10.0), SIMPLE_KERNEL)], ids=["pca", "grey_world", "simple"])
def test_headroom_of_the_wave_sums(gpu_pipe, oracle, method, params, kernel):
    """1024 x 512 blown_with_patch as bayer_rggb8 with stats_blocks = 8: eight wave tasks of 128 row pairs, each summing b^2 and
    r^2 to within 3 % of 2^32 (tests/test_wb_degenerate_cases.py).  One frame and a batch of two."""
    w, h = D.HEADROOM_SIZE
    gpu_pipe.set_tunable("stats_blocks", D.HEADROOM_STATS_BLOCKS)
    configure(gpu_pipe, cfg(wb=True, wb_method=method, **params))
    f = D.frame("blown_with_patch", "bayer_rggb8", w, h)
    g = D.frame("blown", "bayer_rggb8", w, h)
    for frames, single in (([f], True), ([f, g], False)):
        log = run_frames(gpu_pipe, oracle, method, params, "bayer_rggb8", frames, None, "headroom %s x %d" % (method, len(frames)),
                         single=single, kernels=[kernel])
        grids = [r["grid"] for r in log.records() if r["name"] == kernel]
        assert grids == [(8, len(frames))], log.text


# ---- the reference's model on the device --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_frames(form, size):
    frames = D.reference_model_frames(form, size, 16)
    return frames


@pytest.mark.parametrize("form,size", D.REFERENCE_MODEL_FORMS, ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_reference_model_single_frames(gpu_pipe, oracle, form, size):
    params = dict(wb_bright=0.8, wb_dark=0.2)
    configure(gpu_pipe, cfg(wb=True, wb_method="ccc", wb_temporal=False, **params))
    occ = set_model(gpu_pipe, oracle, "default")
    frames = model_frames(form, size)[:3]
    for i, f in enumerate(frames):
        e = D.expected(oracle, "ccc", params, form, f, occ)
        if i == 0 and size == (720, 540):
            assert e.estimate["track"][0:2] == [111, 139]
        got = gpu_pipe.process(f, form)
        w = "default.bin %s frame %d" % (form, i)
        check_estimate(w, "ccc", e.estimate, gpu_pipe.get_white_balance_info(1)[0], gpu_pipe.get_ccc_track(1)[0])
        assert_images_equal(got, e.image, w)


@pytest.mark.parametrize("lds", [False, True], ids=["atomic", "lds"])
@pytest.mark.parametrize("n", [1, 4, 7, 9, 16])
def test_reference_model_batches(gpu_pipe, oracle, n, lds):
    """Batches of 1 and 4 frames run one-wave transforms, larger ones the 16-column transforms; up to 8 frames fold the arg-max into
    the finalisation, 9 and 16 launch it; ccc_lds_hist_min = 1 sends every size through the LDS histogram."""
    params = dict(wb_bright=0.8, wb_dark=0.2)
    form, size = D.REFERENCE_MODEL_FORMS[n % len(D.REFERENCE_MODEL_FORMS)] if n != 16 else D.REFERENCE_MODEL_FORMS[0]
    configure(gpu_pipe, cfg(wb=True, wb_method="ccc", wb_temporal=False, **params))
    occ = set_model(gpu_pipe, oracle, "default")
    gpu_pipe.set_tunable("ccc_lds_hist_min", 1 if lds else 1000000)
    kernels = ["ccc_hist_lds_kernel" if lds else "ccc_hist_kernel", "ccc_fft_rows16_kernel<%d>" % (4 if n <= 4 else 16)]
    forbidden = ["ccc_hist_kernel" if lds else "ccc_hist_lds_kernel"] + (["ccc_argmax_kernel"] if n <= 8 else [])
    if n > 8:
        kernels.append("ccc_argmax_kernel")
    run_frames(gpu_pipe, oracle, "ccc", params, form, list(model_frames(form, size)[:n]), occ, "default.bin %s x %d" % (form, n),
               single=False, kernels=kernels, forbidden=forbidden)


@pytest.mark.parametrize("model,track", [("default", [166, 106]), ("synthetic", [0, 0])])
def test_empty_histogram_known_answers(gpu_pipe, oracle, model, track):
    """Every pixel masked: the response is the bias plane -- the reference's peaks at (166, 106); the synthetic model's is all
    zeros, and the first maximum in row-major order, (0, 0), decides alone."""
    import torch
    params = dict(wb_bright=0.2, wb_dark=0.8)
    configure(gpu_pipe, cfg(wb=True, wb_method="ccc", wb_temporal=False, **params))
    occ = set_model(gpu_pipe, oracle, model)
    frames = [D.frame(k, "bayer_grbg8", 720, 540) for k in ("flat_grey", "zero_channel", "blown_with_patch")]
    for n in (1, 3, 9):
        batch = (frames * 3)[:n]
        gpu_pipe.apply_device(torch.from_numpy(np.stack(batch)).cuda(), "bayer_grbg8")
        got = gpu_pipe.get_ccc_track(n)
        assert got.tolist() == [track * 2] * n, (model, n, got.tolist())
    run_frames(gpu_pipe, oracle, "ccc", params, "bayer_grbg8", frames, occ, "empty histogram " + model)
