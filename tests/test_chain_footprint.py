"""The footprint of the undistortion in its source image (rip_debug_chain_footprint on a RIP_DEVICE_NONE handle, i.e. the
host compiler rip_host.cpp compile_remap_footprint): the fused Bayer chain in front of the remap computes only these items,
so every tap cv::remap takes -- all four bilinear taps of every destination pixel, border pixels included -- must lie inside
it, after the 180-degree flip too.  No GPU needed."""
import numpy as np
import pytest

from helpers import cfg, oracle_maps
from raw_image_pipeline_amd import synth


def shifted_camera(w, h):
    cam = synth.camera_model(w, h)
    K = list(cam["K"])
    K[2] += 0.07 * w   # principal point off centre: the footprint is no longer symmetric
    K[5] -= 0.05 * h
    cam["K"] = K
    P = list(cam["P"])
    P[2], P[6] = K[2], K[5]
    cam["P"] = P
    return cam


CALIBRATIONS = {
    "balance0": dict(balance=0.0, fov_scale=1.0),
    "balance0.5": dict(balance=0.5, fov_scale=1.0),
    "balance1": dict(balance=1.0, fov_scale=1.0),
    "fov0.6": dict(balance=0.0, fov_scale=0.6),
    "fov1.4": dict(balance=0.0, fov_scale=1.4),
    "shifted": dict(balance=0.0, fov_scale=1.0, shifted=True),
}


def expected_hull(mx, my, rows, cols, flip_angle):
    """Per row pair of the chain's input: the hull [lo, hi) of the 4-pixel groups holding an in-bounds tap of cv::remap's
    quantised map (cvRound(m * 32) >> 5, saturated to 16 bits), in the chain's coordinates."""
    fx = mx.astype(np.float64).ravel() * 32
    fy = my.astype(np.float64).ravel() * 32
    ok = np.isfinite(fx) & np.isfinite(fy) & (np.abs(fx) < 2 ** 31) & (np.abs(fy) < 2 ** 31)
    sx = np.clip(np.rint(fx[ok]).astype(np.int64) >> 5, -32768, 32767)
    sy = np.clip(np.rint(fy[ok]).astype(np.int64) >> 5, -32768, 32767)
    pairs, groups = rows // 2, cols // 4
    lo = np.full(pairs, np.iinfo(np.int64).max, np.int64)
    hi = np.full(pairs, -1, np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            ty, tx = sy + dy, sx + dx
            m = (ty >= 0) & (ty < rows) & (tx >= 0) & (tx < cols)
            pr, g = ty[m] // 2, tx[m] // 4
            if flip_angle == 180:
                pr, g = pairs - 1 - pr, groups - 1 - g
            np.minimum.at(lo, pr, g)
            np.maximum.at(hi, pr, g)
    iv = np.zeros((pairs, 2), np.int64)
    hit = hi >= 0
    iv[hit, 0], iv[hit, 1] = lo[hit], hi[hit] + 1
    return iv


def load(host_pipe, w, h, calib):
    cam = shifted_camera(w, h) if calib.get("shifted") else synth.camera_model(w, h)
    c = cfg(undistort=True, cam=cam, balance=calib["balance"], fov_scale=calib["fov_scale"])
    synth.load_camera(host_pipe, cam)
    host_pipe.set_undistortion(True)
    host_pipe.set_undistortion_balance(c["balance"])
    host_pipe.set_undistortion_fov_scale(c["fov_scale"])
    return c


@pytest.mark.parametrize("size", [(2448, 2048), (3840, 2160), (640, 480)])
@pytest.mark.parametrize("calib", list(CALIBRATIONS))
def test_every_remap_tap_lies_inside_the_footprint(host_pipe, oracle, size, calib):
    w, h = size
    c = load(host_pipe, w, h, CALIBRATIONS[calib])
    mx, my = oracle_maps(oracle, c)
    assert mx.shape == (h, w)
    for flip in (0, 180):
        info, iv = host_pipe.debug_chain_footprint(h, w, flip)
        assert info["dense_items"] == (h // 2) * (w // 4)
        want = expected_hull(mx, my, h, w, flip)
        # exactly the hull of the taps: a superset is safe, but the walk is meant to be this one
        bad = np.nonzero((iv != want).any(axis=1))[0]
        assert bad.size == 0, "flip %d, row pairs %s: walked %s, taps %s" % (flip, bad[:5], iv[bad[:5]].tolist(), want[bad[:5]].tolist())
        assert info["footprint_items"] == int((iv[:, 1] - iv[:, 0]).sum())
        assert info["row_pairs"] == int((iv[:, 1] > iv[:, 0]).sum())
        assert info["last_walked"] == 0  # no frame ran on this handle


def test_config2_footprint_is_about_four_fifths_of_the_frame(host_pipe):
    """The headline calibration (balance 0, fov 1): the remap never samples the corners, 21.5 % of the items."""
    w, h = 2448, 2048
    load(host_pipe, w, h, CALIBRATIONS["balance0"])
    info, iv = host_pipe.debug_chain_footprint(h, w, 180)
    frac = info["footprint_items"] / info["dense_items"]
    assert abs(frac - 0.785) <= 0.01, frac
    # all but a few row pairs at the top and the bottom hold a tap at this calibration
    assert h // 2 - 8 <= info["row_pairs"] <= h // 2


def test_flip_mirrors_the_footprint(host_pipe):
    w, h = 640, 480
    load(host_pipe, w, h, CALIBRATIONS["shifted"])
    i0, iv0 = host_pipe.debug_chain_footprint(h, w, 0)
    i1, iv1 = host_pipe.debug_chain_footprint(h, w, 180)
    assert i0["footprint_items"] == i1["footprint_items"] < i0["dense_items"]
    groups = w // 4
    mirrored = np.stack([groups - iv0[::-1, 1], groups - iv0[::-1, 0]], axis=1)
    empty = iv0[::-1, 1] <= iv0[::-1, 0]
    mirrored[empty] = 0
    assert np.array_equal(iv1, mirrored)


def test_footprint_export_rejects_what_the_fast_kernel_does_not_walk(host_pipe):
    from raw_image_pipeline_amd import RipError
    load(host_pipe, 64, 48, CALIBRATIONS["balance0"])
    for args in ((48, 64, 90), (47, 64, 0), (48, 62, 0)):
        with pytest.raises((RipError, ValueError)):
            host_pipe.debug_chain_footprint(*args)
