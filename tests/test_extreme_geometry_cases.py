"""The case list of tests/extreme_geometry_cases.py, checked on the CPU before any GPU time is spent: it is closed over the size
clauses (every clause has a case on each of its sides), the oracle alone runs every case, and what the oracle expects is
non-degenerate -- an undistorted image is mostly image, every expectation holds at least 64 byte values, every white balance
moves the image, and the coordinate saturation of cv::remap decides pixels where a case says it does."""
import numpy as np
import pytest

import extreme_geometry_cases as X
from helpers import oracle_maps, oracle_run


def test_the_list_is_closed_over_the_clauses():
    seen = {}
    for c in X.CASES:
        assert c.crosses, c.name
        for clause, side in c.crosses:
            seen.setdefault(clause, set()).add(side)
    for clause, (_, _, sides) in X.CLAUSES.items():
        assert seen.get(clause, set()) == set(sides), "%s: cases on %s, sides %s" % (clause, sorted(seen.get(clause, ())), sides)


def test_the_shapes_stage_sets_inputs_and_layouts_are_spread_over_the_chain_cases():
    chain = X.family("chain")
    sizes = {c.size for c in chain}
    wide = {(65532, 8), (65536, 8), (262140, 4), (262144, 4), (262148, 6), (70001, 5)}
    tall = {(8, 65534), (8, 65536), (4, 131070), (4, 131072), (6, 131076), (5, 70001)}
    assert wide | tall <= sizes
    assert {c.stages for c in chain} >= {"debayer", "memory", "full"}
    assert {c.flip for c in chain} >= {0, 90, 180, 270}
    assert {c.wb for c in chain} >= {"grey_world", "pca", "simple", "ccc"}
    encodings = {c.encoding for c in chain}
    assert encodings >= {"bayer_rggb8", "bayer_grbg8", "bayer_gbrg8", "bayer_bggr8", "bgr8", "mono8", "bayer_rggb16", "bayer_rggb12p"}
    assert any(c.method == "mht" for c in chain)
    for layouts in ({"tight"}, {"pitch16"}, {"pitch_odd", "base_off"}):   # three resident frames, each on a wide and on a tall frame
        for long_side in (0, 1):
            assert any(c.layout in layouts and c.n == 3 and c.size[long_side] > c.size[1 - long_side] for c in chain), (layouts, long_side)
    # the kernels the geometry clauses select: every chain kernel and every statistics kernel is expected somewhere
    expected = {k for c in chain for k in c.kernels}
    assert expected >= set(X.CHAIN_KERNELS) | set(X.STATS_KERNELS) | {"demosaic_mht_tile_kernel<*>", "raw16_tile_kernel<StageU16*>", "raw16_tile_kernel<StagePacked<*>"}


def test_the_undistortion_cases_cover_both_axes_and_both_routes():
    und = X.family("undistort")
    assert {c.size for c in und} >= {(65532, 8), (65536, 8), (65537, 8), (8, 65534), (8, 65536)}
    assert {c.encoding for c in und} >= {"bayer_rggb8", "bgr8", "mono8"}
    assert sum(1 for c in und if c.extra.get("host_plan")) >= 4 and any(c.extra.get("saturates") for c in und)
    fp = X.family("footprint")
    assert {c.size for c in fp} >= {(262140, 8), (262144, 8), (8, 131070), (8, 131072)}
    assert {c.extra["walk"] for c in fp} == {"footprint", "dense"}
    for c in und + fp:   # every frame stays at 2 Mpx or less (only the 2^22-side cases are larger)
        assert c.size[0] * c.size[1] <= 2100000, c.name
    for c in X.CASES:
        if c.family != "limit" and not X.refused(c):
            assert c.size[0] * c.size[1] <= 2100000 and max(c.size) < X.SIDE_LIMIT, c.name


def test_the_refusals_lie_outside_the_documented_domain():
    for c in X.CASES:
        if not X.refused(c):
            continue
        w, h = c.size
        if c.family == "resize":
            assert max(c.size + c.target) > X.RESIZE_LIMIT, c.name
        elif "pitch" in c.extra:
            assert c.extra["pitch"] >= X.PITCH_LIMIT
        else:
            assert max(w, h) > X.SIDE_LIMIT or w * h * 3 >= 1 << 32, c.name
    at = [c for c in X.family("resize") if not X.refused(c)]
    assert all(max(c.size + c.target) == X.RESIZE_LIMIT for c in at) and {c.extra["interp"] for c in at} == {"linear", "area"}


def outside_fraction(O, case):
    """The share of destination pixels whose taps all lie outside the source: the border constant."""
    mx, my = oracle_maps(O, X.configuration(case))
    w, h = case.size
    sx = np.clip(np.rint(mx.astype(np.float32) * np.float32(32.0)).astype(np.int64) >> 5, -32768, 32767)
    sy = np.clip(np.rint(my.astype(np.float32) * np.float32(32.0)).astype(np.int64) >> 5, -32768, 32767)
    return float(((sx >= w) | (sx + 1 < 0) | (sy >= h) | (sy + 1 < 0)).mean())


def distinct(a):
    """How many byte values (or 16- / 32-bit patterns of a float format) an array holds."""
    a = np.asarray(a)
    return int(np.count_nonzero(np.bincount(a.ravel(), minlength=256))) if a.dtype == np.uint8 else np.unique(a).size


RUNNABLE = [c for c in X.CASES if not X.refused(c)]


@pytest.mark.parametrize("case", RUNNABLE, ids=X.case_id)
def test_the_oracle_runs_the_case_and_its_expectation_is_not_degenerate(oracle, case):
    images = X.expected_images(oracle, case)
    assert len(images) == case.n
    w, h = case.size
    if case.family in ("undistort", "footprint"):
        cw, ch = case.calib or case.size
        shape = (ch, cw)
    else:
        shape = (w, h) if case.flip in (90, 270) else (h, w)
    for e in images:
        assert e.shape[:2] == shape and e.dtype == np.uint8, (case.name, e.shape)
        assert distinct(e) >= 64, "%s: %d distinct byte values" % (case.name, distinct(e))
    assert len({e.tobytes() for e in images}) == case.n, "%s: the frames of the batch are alike" % case.name
    if case.family in ("output", "resize"):
        for d in X.delivered(oracle, case, images):
            assert distinct(d) >= 64, case.name
    if case.family in ("undistort", "footprint"):
        out = outside_fraction(oracle, case)
        assert out <= 0.5, "%s: %.1f %% of the image is the border constant" % (case.name, 100 * out)
        if case.family == "undistort":
            assert out > 0.01, "%s: no border pixels to get wrong (%.2f %%)" % (case.name, 100 * out)
    if case.extra.get("saturates"):
        assert X.saturated_fraction(oracle, case) > 0.25, case.name
    if case.wb is not None and case.encoding != "mono8" and not case.extra.get("sequence"):
        # the gains differ from identity: the oracle's image without the white balance is another one
        off = X.expected_images(oracle, case._replace(wb=None, n=1))[0]
        assert not np.array_equal(off, images[0]), "%s: the white balance changes nothing" % case.name
    if case.extra.get("sequence"):
        assert not np.array_equal(images[0], oracle_run(oracle, X.configuration(case._replace(wb=None)), np.ascontiguousarray(X.frames(case)[0]), case.encoding)[0])
