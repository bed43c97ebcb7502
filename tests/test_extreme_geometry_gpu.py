"""Frames with a side past 65535 and at the limits of the accepted domain, HIP against the CPU oracle at tolerance 0
(tests/extreme_geometry_cases.py; PARITY.md "Geometry limits").

Every case records its launch log and asserts the kernel its size clause says must run on that side, and that the one the clause
excludes did not.  Resident frames are strided views of a sentinel-filled buffer (helpers.device_batch), so a stray write into the
input fails the case.  The last test of the file checks that every case of the list was compared."""
import re

import numpy as np
import pytest

import extreme_geometry_cases as X
import output_variant_cases as OV
import packed_reference as PKR
from helpers import SENTINEL, assert_images_equal, assert_launched, cfg, configure, device_batch, oracle_run
from raw_image_pipeline_amd import RawImagePipeline, synth

pytestmark = pytest.mark.gpu

COMPARED = []


def prepare(pipe, case):
    """The configuration of a case on a handle."""
    configure(pipe, X.configuration(case))
    if case.method == "mht":
        pipe.set_debayer_method("mht")
    if "range16" in case.extra:
        pipe.set_debayer_16bit(True)
        pipe.set_debayer_16bit_range(*case.extra["range16"])
    if case.extra.get("sequence"):
        pipe.set_ccc_model(*synth.ccc_model())
        pipe.set_ccc_kalman_model(1.0, 10.0)
        pipe.reset_white_balance_temporal_consistency()


def run(pipe, case, frames):
    """The frames of a case through the handle: host frames one process() call each, resident frames as one batch in the case's
    layout.  Returns (images, launch log)."""
    import torch
    w, h = case.size
    with pipe.launch_log() as log:
        if case.layout == "host":
            out = []
            for f in frames:
                if "packed" in case.extra:
                    out.append(pipe.process(PKR.pack(X.samples16(case, f), case.extra["packed"]), case.encoding, width=w))
                elif "range16" in case.extra:
                    out.append(pipe.process(X.samples16(case, f), case.encoding))
                else:
                    out.append(pipe.process(np.ascontiguousarray(f), case.encoding))
        else:
            batch = device_batch(np.stack(frames), case.layout, np.random.default_rng(len(case.name)))
            got = pipe.apply_device(batch.view, case.encoding)
            batch.check_padding(case.name)
            torch.cuda.synchronize()
            out = list(got.cpu().numpy())
    return out, log


def compare(oracle, case, out, log):
    want = X.expected_images(oracle, case)
    assert len(out) == len(want) == case.n
    for i, (g, e) in enumerate(zip(out, want)):
        assert_images_equal(g.reshape(e.shape), e, "%s frame %d/%d" % (case.name, i, case.n))
    assert_launched(log, case.kernels, case.forbidden, case.name)


# ---- 1. chain, statistics and demosaic kernels, no undistortion ------------------------------------------------------------------
@pytest.mark.parametrize("case", X.family("chain"), ids=X.case_id)
def test_chain_statistics_and_demosaic_kernels(gpu_pipe, oracle, case):
    prepare(gpu_pipe, case)
    out, log = run(gpu_pipe, case, X.frames(case))
    compare(oracle, case, out, log)
    COMPARED.append(case.name)


# ---- 2. undistortion -----------------------------------------------------------------------------------------------------------
PLAN_KEYS = ("tiles_x", "tiles_y", "border_pixels", "max_lds_bytes", "max_rect_w", "max_rect_h")


@pytest.mark.parametrize("case", X.family("undistort"), ids=X.case_id)
def test_undistortion_on_both_sides_of_the_65535_bound(gpu_pipe, oracle, monkeypatch, case):
    """Tiled, ring and fused remap with the border list inside the bound, the plain gather -- border pixels included -- outside;
    where the case asks for it, the plan compiled on the device against the host compiler's (RIP_PLAN_ON_HOST=1)."""
    w, h = case.size
    frames = X.frames(case)
    prepare(gpu_pipe, case)
    out, log = run(gpu_pipe, case, frames)
    compare(oracle, case, out, log)
    if case.extra.get("host_plan"):
        monkeypatch.setenv("RIP_PLAN_ON_HOST", "1")
        host = RawImagePipeline(False, "", "", "", device=0)
        monkeypatch.delenv("RIP_PLAN_ON_HOST")
        prepare(host, case)
        out_h, log_h = run(host, case, frames)
        for i in range(case.n):
            assert_images_equal(out_h[i], out[i], "%s frame %d, host plan vs device plan" % (case.name, i))
        assert_launched(log_h, case.kernels, case.forbidden, case.name + " (host plan)")
        info_d, info_h = gpu_pipe.debug_plan_info(h, w), host.debug_plan_info(h, w)
        assert info_d["on_device"] == 1 and info_h["on_device"] == 0, (info_d, info_h)
        for key in PLAN_KEYS:
            assert info_d[key] == info_h[key], (case.name, key, info_d, info_h)
        inside = all(side != "above" for _, side in case.crosses)
        assert (info_d["border_pixels"] > 0) == inside, (case.name, info_d)   # the list exists inside the bound only
    COMPARED.append(case.name)


@pytest.mark.parametrize("case", X.family("footprint"), ids=X.case_id)
def test_footprint_walk_on_both_sides_of_its_bound(gpu_pipe, oracle, case):
    """A calibration smaller than the image: the chain in front of the remap walks the item list while rows / 2 and cols / 4 fit 16
    bits, and every item past it.  rip_debug_chain_footprint's last_walked says which walk ran; past the bound the hook refuses
    the geometry by the same clause, and last_walked is read through a geometry it takes."""
    import torch
    w, h = case.size
    frames = X.frames(case)
    prepare(gpu_pipe, case)
    gpu_pipe.set_tunable("chain_footprint", 1)
    batch = device_batch(np.stack(frames), case.layout, np.random.default_rng(7))
    with gpu_pipe.launch_log() as log:
        got = gpu_pipe.apply_device(batch.view, case.encoding)
        torch.cuda.synchronize()
    batch.check_padding(case.name)
    dense_items = (h // 2) * (w // 4)
    if case.extra["walk"] == "footprint":
        info, iv = gpu_pipe.debug_chain_footprint(h, w, case.flip)
        assert info["dense_items"] == dense_items
        assert 0 < info["last_walked"] == info["footprint_items"] < 0.95 * dense_items, (case.name, info)
        if any(side == "at" for _, side in case.crosses):   # flip 180 lists the far end of the source: the field's last value, 65534
            assert case.flip == 180
            if w > h:
                assert int(iv[:, 1].max()) - 1 == w // 4 - 1 == 65534, (case.name, int(iv[:, 1].max()))
            else:
                assert int(np.flatnonzero(iv[:, 1] > iv[:, 0]).max()) == h // 2 - 1 == 65534, case.name
    else:
        with pytest.raises(ValueError):
            gpu_pipe.debug_chain_footprint(h, w, case.flip)
        small = (64, 8) if w > h else (8, 64)
        assert gpu_pipe.debug_chain_footprint(small[1], small[0], case.flip)[0]["last_walked"] == dense_items, case.name
        prepare(gpu_pipe, case)
    compare(oracle, case, list(got.cpu().numpy()), log)
    # the same frames with the footprint switched off: the dense walk, the same bytes
    gpu_pipe.set_tunable("chain_footprint", 0)
    dense = gpu_pipe.apply_device(batch.view, case.encoding)
    torch.cuda.synchronize()
    assert torch.equal(got, dense), "%s: footprint walk differs from the dense walk on %d bytes" % (case.name, int((got != dense).sum()))
    COMPARED.append(case.name)


# ---- 3. delivered frames ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.family("output"), ids=X.case_id)
def test_output_formats_past_one_trip_of_the_row_loop(rip_lib, oracle, case):
    import torch
    from test_output_format_gpu import Destination
    w, h = case.size
    fmt = case.extra["fmt"]
    frames = X.frames(case)
    want = np.stack(X.delivered(oracle, case, X.expected_images(oracle, case)))
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, cfg())
    pipe.set_output_format(fmt)
    pipe.set_output_normalization(*OV.NORM)
    batch = device_batch(np.stack(frames), case.layout, np.random.default_rng(3))
    dst = Destination(fmt, case.n, h, w, pitch=case.extra["pitch"])
    with pipe.launch_log() as log:
        out = pipe.apply_device(batch.view, "bgr8", out=dst.view)
    assert out is dst.view and pipe.last_encoding == fmt
    dst.check(want, case.name)
    batch.check_padding(case.name)
    rec = [r for r in log.records() if r["name"].startswith("output_convert_kernel")]
    assert len(rec) == 1 and rec[0]["name"] == OV.KERNEL_OF_FORMAT[fmt] and rec[0]["grid"][1] == min(h, 65535), log.text
    COMPARED.append(case.name)


def ordinary_frame_still_works(pipe, oracle):
    """After a refusal: every output stage off, one small frame against the oracle."""
    pipe.set_output_size(0, 0)
    pipe.set_output_format("native")
    c = cfg(wb=True, wb_method="grey_world", gamma=True)
    configure(pipe, c)
    f = synth.gen_frame(64, 48, "bayer_rggb8", seed=5, kind="scene")
    assert_images_equal(pipe.process(f, "bayer_rggb8"), oracle_run(oracle, c, f, "bayer_rggb8")[0], "an ordinary frame after the refusal")


@pytest.mark.parametrize("case", X.family("resize"), ids=X.case_id)
def test_resize_at_its_side_limit_and_refused_past_it(rip_lib, oracle, case):
    """Targets and sources up to 16384 per side run (linear, the 2 x 2 mean, area); anything larger -- the sizes at which
    gridDim.y would pass 65535 among them -- is RIP_ERR_INVALID_ARGUMENT before a launch."""
    import torch
    w, h = case.size
    tw, th = case.target
    frames = np.stack(X.frames(case))
    pipe = RawImagePipeline(False, "", "", "", device=0)
    configure(pipe, cfg())
    pipe.set_output_interpolation(case.extra["interp"])
    dev = torch.from_numpy(frames).cuda()
    if X.refused(case):
        with pipe.launch_log() as log:
            with pytest.raises(ValueError, match=X.refused(case)):
                pipe.set_output_size(tw, th)
                pipe.apply_device(dev, case.encoding)
        assert not log.records(), log.text
        ordinary_frame_still_works(pipe, oracle)
    else:
        pipe.set_output_size(tw, th)
        want = X.delivered(oracle, case, X.expected_images(oracle, case))
        with pipe.launch_log() as log:
            got = pipe.apply_device(dev, case.encoding)
            torch.cuda.synchronize()
        got = got.cpu().numpy()
        for i in range(case.n):
            assert_images_equal(got[i], want[i], "%s frame %d" % (case.name, i))
        rec = [r for r in log.records() if r["name"].startswith(("resize_kernel", "area_reduce_kernel"))]
        assert [r["name"] for r in rec] == list(case.kernels) and rec[0]["grid"][1] == case.extra["grid_y"], log.text
    COMPARED.append(case.name)


# ---- 4. the accepted limits themselves -------------------------------------------------------------------------------------------
def pitched_view(frame, pitch):
    """One frame on the device as a [1, rows, cols] view whose rows lie `pitch` bytes apart in a sentinel-filled buffer."""
    import torch
    rows, cols = frame.shape
    host = np.full(pitch * (rows - 1) + cols + 16, SENTINEL, np.uint8)
    np.lib.stride_tricks.as_strided(host, (rows, cols), (pitch, 1))[...] = frame
    backing = torch.from_numpy(host).cuda()
    return torch.as_strided(backing, (1, rows, cols), (pitch * rows, pitch, 1)), backing, torch.from_numpy(host)


@pytest.mark.parametrize("case", X.family("limit"), ids=X.case_id)
def test_the_limits_of_the_domain(gpu_pipe, oracle, case):
    """A side of exactly 2^22 and a pitch of 2^24 - 16 are processed and equal the oracle; one past either, and a frame of 4 GiB,
    are refused with the documented message, enqueue nothing and leave the handle working."""
    import torch
    w, h = case.size
    if X.refused(case):
        match = re.escape(X.refused(case))
        with gpu_pipe.launch_log() as log:
            if "pitch" in case.extra:
                view, _, _ = pitched_view(X.frames(case)[0], case.extra["pitch"])
                with pytest.raises(ValueError, match=match):
                    gpu_pipe.apply_device(view, case.encoding)
            else:
                lazy = np.zeros((h, w), np.uint8)   # never touched: the refusal comes before any byte of the frame is read
                with pytest.raises(ValueError, match=match):
                    gpu_pipe.process(lazy, case.encoding)
                with pytest.raises(ValueError, match=match):
                    gpu_pipe.query_output(h, w, 1, case.encoding)
                if not case.extra.get("lazy"):
                    with pytest.raises(ValueError, match=match):
                        gpu_pipe.apply_device(torch.empty((1, h, w), dtype=torch.uint8, device="cuda"), case.encoding)
        assert not log.records(), log.text
        ordinary_frame_still_works(gpu_pipe, oracle)
    elif "pitch" in case.extra:
        prepare(gpu_pipe, case)
        view, backing, before = pitched_view(X.frames(case)[0], case.extra["pitch"])
        with gpu_pipe.launch_log() as log:
            got = gpu_pipe.apply_device(view, case.encoding)
            torch.cuda.synchronize()
        assert torch.equal(backing.cpu(), before), "%s: the input buffer was written" % case.name
        compare(oracle, case, list(got.cpu().numpy()), log)
    else:
        prepare(gpu_pipe, case)
        out, log = run(gpu_pipe, case, X.frames(case))
        compare(oracle, case, out, log)
    COMPARED.append(case.name)


def test_every_case_was_compared():
    """Runs after the cases above (file order): none of them may have been skipped or have left before its last comparison."""
    assert sorted(COMPARED) == sorted(c.name for c in X.CASES), "compared %d of %d cases" % (len(COMPARED), len(X.CASES))
