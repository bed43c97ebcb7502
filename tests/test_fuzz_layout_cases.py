"""The generators of tests/test_fuzz_layout_gpu.py, checked without a GPU: a fuzz that silently stops reaching a path is worse
than none.  At the default case counts every batch layout, batch length, flip, pattern and tile-edge class must occur, the
footprint family must mostly land on geometries where the fused chain walks the item list (host compiler, RIP_DEVICE_NONE),
and the helper that states the CPU expectation of an MHT frame is pinned against the numpy restatement."""
import numpy as np
import pytest

import fuzz_layout_cases as G
from helpers import LAYOUTS, SENTINEL, batch_geometry, cfg, expected_mht
from mht_reference import flip as flip_image, mht_reference
from raw_image_pipeline_amd import synth

DEFAULT_CASES = 60   # what RIP_FUZZ_CASES defaults to; the conditions below are stated for it whatever the environment says


def test_mht_family_reaches_every_layout_batch_flip_pattern_and_edge_class():
    cases = [G.mht_case(k) for k in range(DEFAULT_CASES)]
    assert cases[7] == G.mht_case(7)   # a pure function of the seed
    assert {c["layout"] for c in cases} == set(LAYOUTS)
    assert {c["n"] for c in cases} == set(G.MHT_BATCHES)
    assert {c["flip"] for c in cases} == set(G.FLIPS)
    assert {c["pattern"] for c in cases} == set(G.PATTERNS)
    assert {c["tap"] for c in cases} == {True, False}
    for cls in G.MHT_WIDTH_CLASSES:
        assert any(c["w"] in cls for c in cases), "no width in %s" % (cls,)
    for cls in G.MHT_HEIGHT_CLASSES:
        assert any(c["h"] in cls for c in cases), "no height in %s" % (cls,)
    for c in cases:
        assert c["w"] >= 3 and c["h"] >= 3
        if min(c["w"], c["h"]) < 9:   # demosaic and flip only
            assert not any(c["c"][k] for k in ("wb", "cc", "gamma", "vig", "ce", "undistort")), c
        ow, oh = (c["h"], c["w"]) if c["flip"] in (90, 270) else (c["w"], c["h"])
        assert (c["c"]["cam"]["width"], c["c"]["cam"]["height"]) == (ow, oh)
    # the handle's padded MHT image in front of the vectorised colour kernels
    padded = [c for c in cases if c["w"] % 4 == 0 and c["w"] * 3 % 16 != 0 and not c["tap"]]
    assert len(padded) >= 5, len(padded)
    assert any(any(c["c"][k] for k in ("wb", "cc", "gamma", "vig", "ce", "undistort")) for c in padded)
    # more than one frame group on sizes with interior tiles (the register prefetch of frame f + groups)
    grouped = [c for c in cases if c["n"] >= 5 and c["w"] >= 200 and c["h"] >= 100]
    assert len(grouped) >= 5, len(grouped)
    assert {c["c"]["wb_method"] for c in cases if c["c"]["wb"]} == {"grey_world", "pca", "simple"}
    assert any(not c["c"]["wb"] for c in cases)


def test_layout_family_reaches_every_encoding_in_three_layouts_and_every_batch_length():
    cases = [G.layout_case(k) for k in range(DEFAULT_CASES)]
    for enc in G.LAYOUT_ENCODINGS:
        layouts = {c["layout"] for c in cases if c["encoding"] == enc}
        assert len(layouts) >= 3, (enc, layouts)
    assert {c["n"] for c in cases} == set(G.LAYOUT_BATCHES)
    assert {c["layout"] for c in cases} == set(LAYOUTS)
    for c in cases:
        assert c["n"] * c["w"] * c["h"] <= G.LAYOUT_PIXEL_CAP and c["w"] >= 9 and c["h"] >= 9
        assert c["w"] <= (200 if c["n"] == 33 else 400) and c["h"] <= (120 if c["n"] == 33 else 300)
        assert not (c["encoding"] == "mono8" and c["c"]["vig"])
    # pitched colour input on the vectorised kernels' geometry: cols % 4 == 0 and a dword-aligned pitch
    assert any(c["encoding"] in ("bgr8", "rgb8") and c["layout"] == "pitch16" and c["w"] % 4 == 0 for c in cases)


def test_footprint_family_mostly_lands_on_the_item_list(host_pipe):
    cases = [G.footprint_case(k) for k in range(max(8, DEFAULT_CASES // 2))]
    assert {c["n"] for c in cases} == set(G.FOOTPRINT_BATCHES)
    assert {c["layout"] for c in cases} == set(G.FOOTPRINT_LAYOUTS)
    assert {c["flip"] for c in cases} == {"off", 0, 180}
    listed = 0
    for case in cases:
        c = case["c"]
        assert c["undistort"] and (c["vig"] or c["ce"]) and case["w"] % 4 == 0 and case["h"] % 2 == 0
        synth.load_camera(host_pipe, c["cam"])
        host_pipe.set_undistortion(True)
        host_pipe.set_undistortion_balance(c["balance"])
        host_pipe.set_undistortion_fov_scale(c["fov_scale"])
        info, _ = host_pipe.debug_chain_footprint(case["h"], case["w"], c["flip_angle"] if c["flip"] else 0)
        assert info["dense_items"] == (case["h"] // 2) * (case["w"] // 4)
        listed += info["footprint_items"] <= 0.95 * info["dense_items"]
    assert listed * 3 >= len(cases) * 2, "%d of %d cases at or below 0.95 of the dense walk" % (listed, len(cases))
    assert listed < len(cases), "no case falls back to the dense walk"


def test_layout_geometries():
    rng = np.random.default_rng(1)
    for row_bytes, rows in ((300, 7), (301, 8), (903, 5), (64, 4)):
        assert batch_geometry("tight", row_bytes, rows, rng) == (0, row_bytes, row_bytes * rows)
        off, pitch, frame = batch_geometry("pitch16", row_bytes, rows, rng)
        assert off == 0 and pitch % 16 == 0 and 16 <= pitch - row_bytes < 32 and frame == pitch * rows
        off, pitch, frame = batch_geometry("pitch_odd", row_bytes, rows, rng)
        assert off == 0 and 1 <= pitch - row_bytes <= 3 and frame == pitch * rows
        off, pitch, frame = batch_geometry("base_off", row_bytes, rows, rng)
        assert 1 <= off <= 3 and pitch % 4 == 0 and pitch >= row_bytes and frame == pitch * rows
        off, pitch, frame = batch_geometry("frame_gap", row_bytes, rows, rng)
        assert off == 0 and pitch == row_bytes and frame in (pitch * (rows + 1), pitch * (rows + 2), pitch * (rows + 3))
    assert SENTINEL == 0xA5


@pytest.mark.parametrize("size", [(3, 3), (67, 35), (324, 200)])
@pytest.mark.parametrize("angle", [0, 90, 180, 270])
def test_expected_mht_debayered_tap_is_the_flipped_reference(oracle, size, angle):
    w, h = size
    ow, oh = (h, w) if angle in (90, 270) else (w, h)
    pattern = G.PATTERNS[(w + angle // 90) % 4]
    c = cfg(flip=True, flip_angle=angle, wb=True, wb_method="grey_world", cc=True, gamma=True, gamma_k=0.8, vig=True, ce=True, ce_sat=1.2,
            undistort=True, cam=synth.camera_model(ow, oh))
    frame = synth.gen_frame(w, h, pattern, seed=w + angle, kind="scene")
    out, enc, t_deb, t_col = expected_mht(oracle, c, frame, pattern, taps=True)
    assert enc == "bgr8" and out.shape == (oh, ow, 3)
    assert np.array_equal(t_deb.reshape(oh, ow, 3), flip_image(mht_reference(frame, pattern), angle))
    assert t_col.size == out.size
    plain, enc2 = expected_mht(oracle, c, frame, pattern)
    assert enc2 == "bgr8" and np.array_equal(plain, out)
