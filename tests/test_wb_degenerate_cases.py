"""CPU side of the degenerate white-balance cases (tests/wb_degenerate_cases.py; PARITY.md "Degenerate frames"): before any GPU
time is spent, the oracle runs every case to a defined result, the answers on the simplest frames are pinned, every case flagged
"the image proves the estimate" really does, every compared ccc arg-max is decided far above float noise, and the frame that
takes the statistics kernel to the edge of its 32-bit wave sums really gets there."""
import functools

import numpy as np
import pytest

import wb_degenerate_cases as D
from helpers import cfg, oracle_run


# ---- numpy restatements of the apply side of oracle/rip_oracle.c, checked against the oracle in every case they are used for --------
def sat_u8_f(x):
    """sat_u8_f: (int)lrintf(v) clamped to 0..255.  lrintf rounds half to even and gives LONG_MIN for NaN, infinities and
    values beyond the long range (x86-64); the cast keeps the low 32 bits."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(x, np.float32).astype(np.float64))
        bad = ~np.isfinite(r) | (np.abs(r) >= 2.0 ** 63)
        i64 = np.where(bad, -2.0 ** 63, r).astype(np.int64)
    return np.clip(i64.astype(np.int32), 0, 255).astype(np.uint8)


def grey_world_q8(sums):
    """ripo_wb_grayworld: channel sums -> Q8 gains."""
    s = [float(v) for v in sums]
    max_sum = max(s)
    g = [np.float32(0.0) if v < 0.1 else np.float32(max_sum / v) for v in s]
    gmax = max(g)
    if gmax > 0:
        g = [np.float32(v / gmax) for v in g]
    return [int(np.rint(np.float32(v * np.float32(256.0)))) for v in g]


def grey_world_apply(seen, q8):
    out = (seen.astype(np.int64) * np.asarray(q8, np.int64)) >> 8
    return (out & 0xFF).astype(np.uint8)


def solve2(m00, m01, m10, m11, g0, g1):
    f = np.float32
    with np.errstate(all="ignore"):
        det = f(f(m00 * m11) - f(m01 * m10))
        invdet = f(f(1.0) / det)
        i00, i01, i10, i11 = f(m11 * invdet), f(-m01 * invdet), f(-m10 * invdet), f(m00 * invdet)
        return f(f(i00 * g0) + f(i01 * g1)), f(f(i10 * g0) + f(i11 * g1))


def pca_sums(seen):
    b, g, r = (seen[..., c].astype(np.int64) for c in range(3))
    return [int(b.sum()), int((b * b).sum()), int(r.sum()), int((r * r).sum()), int(g.sum())], [int(b.max()), int(r.max()), int(g.max())]


def pca_coeffs(sums, mx):
    """ripo_wb_pca: sums (b, b^2, r, r^2, g) and maxima (b, r, g) -> (c0, c1) of B and of R."""
    f = np.float32
    s = [f(float(v)) for v in sums]
    mb, mr, mg = (f(v) for v in mx)
    cb = solve2(s[1], s[0], f(mb * mb), mb, s[4], mg)
    cr = solve2(s[3], s[2], f(mr * mr), mr, s[4], mg)
    return np.asarray([cb[0], cb[1], cr[0], cr[1]], np.float32)


def pca_apply(seen, co):
    out = seen.copy()
    with np.errstate(all="ignore"):
        for ch, (c0, c1) in ((0, co[0:2]), (2, co[2:4])):
            v = seen[..., ch].astype(np.float32)
            t = (v * v) * np.float32(c0) + v * np.float32(c1)
            t = np.where(t > np.float32(255.0), np.float32(255.0), t)   # THRESH_TRUNC keeps a NaN
            out[..., ch] = sat_u8_f(t)
    return out


def simple_apply(seen, ab):
    out = seen.copy()
    with np.errstate(all="ignore"):
        for ch in range(3):
            out[..., ch] = sat_u8_f(seen[..., ch].astype(np.float32) * np.float32(ab[2 * ch]) + np.float32(ab[2 * ch + 1]))
    return out


def ccc_apply(seen, gains):
    return sat_u8_f(seen.astype(np.float32) * np.asarray(gains, np.float32))


# ---- perturbed estimates -----------------------------------------------------------------------------------------------------
def perturbed_images(O, case, exp):
    """[(class, what, image)] for every perturbed estimate that differs from the true one; asserts first that the restated apply side
    reproduces the oracle's image from the true estimate.  The perturbations: one channel sum off by 2^32 (a wrapped 32-bit
    reduction), a Q8 gain off by one, a (u, v) bin off by one, SimpleWB's low cut one histogram level higher."""
    seen, est, out = exp.seen, exp.estimate, []
    if case.method == "grey_world":
        assert grey_world_q8(est["sums"]) == est["q8"]
        assert np.array_equal(grey_world_apply(seen, est["q8"]), exp.image)
        for c in range(3):
            sums = list(est["sums"])
            sums[c] += 1 << 32
            q8 = grey_world_q8(sums)
            if q8 != est["q8"]:
                out.append(("sum", "sum %d + 2^32" % c, grey_world_apply(seen, q8)))
            q8 = list(est["q8"])
            q8[c] += -1 if q8[c] > 0 else 1
            out.append(("q8", "q8[%d] off by one" % c, grey_world_apply(seen, q8)))
    elif case.method == "pca":
        sums, mx = pca_sums(seen)
        assert D.same_floats(pca_coeffs(sums, mx), est["coeffs"]), (pca_coeffs(sums, mx), est["coeffs"])
        assert np.array_equal(pca_apply(seen, est["coeffs"]), exp.image)
        for k in range(5):
            s = list(sums)
            s[k] += 1 << 32
            co = pca_coeffs(s, mx)
            if not D.same_floats(co, est["coeffs"]):
                out.append(("sum", "sum %d + 2^32" % k, pca_apply(seen, co)))
    elif case.method == "simple":
        assert np.array_equal(simple_apply(seen, est["ab"]), exp.image)
        for c in range(3):
            alpha, beta = float(est["ab"][2 * c]), float(est["ab"][2 * c + 1])
            d = 255.0 / alpha
            lo = -beta / alpha + 1.0   # one level of the fine histogram
            if d - 1.0 <= 0:
                continue
            ab = est["ab"].copy()
            ab[2 * c], ab[2 * c + 1] = 255.0 / (d - 1.0), -lo * 255.0 / (d - 1.0)
            out.append(("cut", "low cut of channel %d one level up" % c, simple_apply(seen, ab)))
    else:
        x, y = est["track"][2:4]
        assert D.same_floats(O.ccc_gains_from_uv(x, y), est["gains"])
        assert np.array_equal(ccc_apply(seen, est["gains"]), exp.image)
        for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            if 0 <= x + dx <= 255 and 0 <= y + dy <= 255:
                g = O.ccc_gains_from_uv(x + dx, y + dy)
                if not D.same_floats(g, est["gains"]):
                    out.append(("uv", "(u, v) + (%d, %d)" % (dx, dy), ccc_apply(seen, g)))
    return out


@functools.lru_cache(maxsize=None)
def ccc_object(model):
    import oracle as O
    filt, bias = D.model_arrays(model)
    return O.CCC(filt, bias)


def run_case(O, case):
    f = D.frame(case.kind, case.form, *case.size)
    occ = ccc_object(case.model) if case.method == "ccc" else None
    return f, D.expected(O, case.method, case.params, case.form, f, occ)


# ---- the tests -----------------------------------------------------------------------------------------------------------------
def test_case_lists():
    assert len(D.CASES) == len({D.case_id(c) for c in D.CASES}) == (9 * 3 + 6 * 2) * 6 * 12
    assert {c.kind for c in D.CASES} == set(D.KINDS) and {c.form for c in D.CASES} == set(D.FORMS)
    assert {c.witness for c in D.CASES} == {"image", "info", "both", "none"}
    # every statistics kernel is reached by the three sizes
    kernels = {(form.startswith("bayer_"), D.expected_stats_kernel(form, size)) for form in D.FORMS for size in D.STAT_SIZES}
    assert kernels == {(True, "stats_fast_kernel<?>"), (True, "stats_generic_kernel"), (False, "stats_color_kernel"), (False, "stats_generic_kernel")}
    for form in D.FORMS:
        assert D.expected_stats_kernel(form, (64, 48)) != "stats_generic_kernel" and D.expected_stats_kernel(form, (51, 33)) == "stats_generic_kernel"
        if form.startswith("bayer_"):
            assert D.expected_stats_kernel(form, (132, 36)) == "stats_fast_kernel<?>"
    # the content is what its name says, in every form
    for form in D.FORMS:
        for w, h in D.STAT_SIZES:
            flat = D.frame("flat_plus_one_pixel", form, w, h)
            assert (flat != 128).sum() == (1 if form.startswith("bayer_") else 2), form
            assert set(np.unique(D.frame("lens_cap", form, w, h))) == {0, 1} and set(np.unique(D.frame("blown", form, w, h))) == {254, 255}
            patch = D.frame("blown_with_patch", form, w, h)
            assert patch.min() < 64 and (patch < 254).sum() <= D.PATCH * D.PATCH * 3


@pytest.mark.parametrize("key", list(D.groups()), ids=D.group_id)
def test_oracle_gives_a_defined_result_and_the_witness_holds(oracle, key):
    """Every case of the group: the oracle returns an image of the frame's size, equal to what its whole pipeline returns with
    only white balance on, and an estimate whose every coefficient is finite or NaN, never infinite.  Where the case says that the image proves the estimate, the oracle's image changes under at least one perturbed
    estimate of every class of perturbation the method has; a case that fails this would have to be dropped, and none is."""
    dropped = []
    for case in D.groups()[key]:
        f, exp = run_case(oracle, case)
        assert exp.image.shape == exp.seen.shape == (case.size[1], case.size[0], 3)
        occ = ccc_object(case.model) if case.method == "ccc" else None
        c = cfg(wb=True, wb_method=case.method, **case.params)
        whole = oracle_run(oracle, c, f, case.form, ccc=occ)[0]
        assert np.array_equal(whole, exp.image), D.case_id(case)
        for k, v in exp.estimate.items():
            assert np.all(np.isfinite(v) | np.isnan(v)) if isinstance(v, np.ndarray) else all(isinstance(i, int) for i in v), (D.case_id(case), k, v)
        perturbed = perturbed_images(oracle, case, exp)   # also checks the restated apply side against the oracle
        if case.witness in ("info", "none"):
            assert (case.witness == "none") == (case.method == "pca")
            continue
        shown = {cls for cls, what, img in perturbed if not np.array_equal(img, exp.image)}
        if not PERTURBATION_CLASSES[case.method] <= shown:
            dropped.append((D.case_id(case), sorted(PERTURBATION_CLASSES[case.method] - shown)))
    assert len(dropped) == 0, dropped


PERTURBATION_CLASSES = {"grey_world": {"sum", "q8"}, "pca": {"sum"}, "simple": {"cut"}, "ccc": {"uv"}}


def test_only_pca_on_frames_of_zeros_and_saturated_values_proves_nothing():
    """pca has no getter, so a case whose image no perturbed sum moves runs for its defined result alone: the black frame (NaN
    coefficients, zeros either way) and the primaries (values 0 and 255 only: 0 stays 0, and the row of maxima pins 255 to 255)."""
    none = [c for c in D.CASES if c.witness == "none"]
    assert len(none) == 2 * len(D.FORMS) * len(D.STAT_SIZES) and all(c.method == "pca" and c.kind in ("black", "primaries") for c in none)
    for method in ("grey_world", "simple", "ccc"):
        assert all(c.witness in ("info", "both") for c in D.CASES if c.method == method)
        assert sum(c.witness == "both" for c in D.CASES if c.method == method) * 3 >= sum(c.method == method for c in D.CASES)


# The answers on 64 x 48 bgr8 frames (PARITY.md "Degenerate frames").  q8: grey-world's Q8 gains; pca: (c0, c1) of B and of R;
# simple: alpha and beta of B.  Constant frames do not depend on the seed; the random ones are those of this module's seeds.
def known(kind, method, **params):
    import oracle as O
    f = D.frame(kind, "bgr8", 64, 48)
    return D.expected(O, method, params, "bgr8", f)


def test_known_answers_black_white_flat(oracle):
    e = known("black", "grey_world", wb_bright=0.8)
    assert e.estimate == dict(q8=[0, 0, 0], sums=[0, 0, 0]) and not e.image.any()
    e = known("black", "pca")
    assert np.isnan(e.estimate["coeffs"]).all() and not e.image.any()
    e = known("black", "simple", wb_percentile=10.0)
    assert list(e.estimate["ab"]) == [255.0, 127.5] * 3 and (e.image == 128).all()

    e = known("white", "grey_world", wb_bright=0.8)
    assert e.estimate["q8"] == [256] * 3 and (e.image == 255).all()
    e = known("white", "pca")
    assert np.isnan(e.estimate["coeffs"]).all()
    assert not e.image[..., 0].any() and not e.image[..., 2].any() and (e.image[..., 1] == 255).all()   # NaN -> 0 on B and R
    e = known("white", "simple", wb_percentile=10.0)
    assert list(e.estimate["ab"]) == [255.0, -64897.5] * 3 and (e.image == 128).all()

    e = known("flat_colour", "grey_world", wb_bright=0.8)   # (200 - 17) * 255 > 204 * 200: every pixel skipped
    assert e.estimate == dict(q8=[0, 0, 0], sums=[0, 0, 0]) and not e.image.any()
    e = known("flat_colour", "grey_world", wb_bright=1.0)
    assert e.estimate["q8"] == [22, 47, 256]
    e = known("flat_colour", "pca")
    assert np.isnan(e.estimate["coeffs"]).all() and not e.image[..., 0].any() and not e.image[..., 2].any() and (e.image[..., 1] == 93).all()
    e = known("flat_colour", "simple", wb_percentile=10.0)
    assert (e.image == 128).all()


def test_known_answers_dead_channel_and_near_singular(oracle):
    e = known("const_channel", "grey_world", wb_bright=0.8)
    assert e.estimate["q8"][0] == 256 and all(135 <= v <= 150 for v in e.estimate["q8"][1:]), e.estimate
    e = known("const_channel", "pca")
    co = e.estimate["coeffs"]
    assert np.isnan(co[0:2]).all() and np.isfinite(co[2:4]).all() and not e.image[..., 0].any() and e.image[..., 2].any()
    e = known("const_channel", "simple", wb_percentile=10.0)
    assert list(e.estimate["ab"][0:2]) == [255.0, -19507.5]

    e = known("flat_plus_one_pixel", "grey_world", wb_bright=0.8)
    assert e.estimate["q8"] == [256] * 3
    e = known("flat_plus_one_pixel", "pca")   # pure cancellation: the determinant is the difference of two products near 2^35
    assert D.same_floats(e.estimate["coeffs"], np.asarray([-0.007751822471618652, 1.9922256469726562, -0.0078125, 2.0], np.float32)), [float(v) for v in e.estimate["coeffs"]]
    e = known("flat_plus_one_pixel", "simple", wb_percentile=10.0)
    assert list(e.estimate["ab"]) == [255.0, -32512.5] * 3 and set(int(v) for v in np.unique(e.image)) == {0, 128, 255}

    e = known("blown", "grey_world", wb_bright=0.8)
    assert e.estimate["q8"] == [256] * 3
    e = known("blown", "simple", wb_percentile=10.0)
    assert list(e.estimate["ab"]) == [127.5, -32321.25] * 3
    co = known("blown", "pca").estimate["coeffs"]
    assert np.isfinite(co).all() and abs(co[0]) < 1e-2 and 0.5 < co[1] < 1.5, co   # ill-conditioned: the draw decides the digits


def test_a_wrapped_sum_shows_on_the_patch_but_not_on_the_plain_blown_frame(oracle):
    """Why blown_with_patch exists: on the plain blown frame pca maps 254 to 254 and 255 to 255 whether or not a sum wrapped.  On
    the headroom frame (the 1024 x 512 rggb mosaic) one wrap of the sum of b^2 takes the coefficients from about (7.0e-4, 0.821)
    to (9.3e-6, 0.998) and moves a thousand pixels of the patch by up to 11 levels."""
    w, h = D.HEADROOM_SIZE
    for kind, shows in (("blown", False), ("blown_with_patch", True)):
        e = D.expected(oracle, "pca", {}, "bayer_rggb8", D.frame(kind, "bayer_rggb8", w, h))
        sums, mx = pca_sums(e.seen)
        assert sums[1] > 1 << 32
        sums[1] -= 1 << 32
        co = pca_coeffs(sums, mx)
        assert not D.same_floats(co, e.estimate["coeffs"])
        moved = int((pca_apply(e.seen, co) != e.image).sum())
        assert (moved >= 500) if shows else (moved == 0), (kind, moved)


# ---- ccc ---------------------------------------------------------------------------------------------------------------------------
def response_of(O, occ, seen):
    hist = occ.histogram(O.resize_linear(seen, 270, 360))
    return hist, occ.response(hist)


@pytest.mark.parametrize("model", D.CCC_MODELS)
def test_ccc_argmax_is_decided_far_above_float_noise(oracle, model):
    """For every ccc case: either the histogram is empty (the response is the bias plane: all zeros for the synthetic model, where
    cv::minMaxLoc's first maximum in row-major order decides alone and is pinned to (0, 0); the reference's bias peak at (166, 106)
    for default.bin), or the gap between the largest and the second largest response is at least 1000 ulp of the largest."""
    occ = ccc_object(model)
    smallest = None
    for case in D.CASES:
        if case.method != "ccc" or case.model != model:
            continue
        f, exp = run_case(oracle, case)
        hist, resp = response_of(oracle, occ, exp.seen)
        flat = np.sort(resp.reshape(-1))
        top, second = float(flat[-1]), float(flat[-2])
        x, y = exp.estimate["track"][0:2]
        assert resp[y, x] == flat[-1], D.case_id(case)
        if not hist.any():
            assert (x, y) == ((0, 0) if model == "synthetic" else (166, 106)), (D.case_id(case), x, y)
            if model == "synthetic":
                assert top == second == 0.0   # all tied: exempt from the gap, pinned to (0, 0)
                assert D.same_floats(exp.estimate["gains"], oracle.ccc_gains_from_uv(0, 0))
                continue
        gap = (top - second) / float(np.spacing(np.float32(abs(top))))
        assert gap >= 1000, "%s: the arg-max is decided by %.1f ulp" % (D.case_id(case), gap)
        smallest = gap if smallest is None else min(smallest, gap)
    assert smallest is not None
    if (0.2, 0.8) in D.CCC_THRESHOLDS:
        empty = [c for c in D.CASES if c.method == "ccc" and c.model == model and (c.params["wb_bright"], c.params["wb_dark"]) == (0.2, 0.8)]
        assert empty and all(not response_of(oracle, occ, run_case(oracle, c)[1].seen)[0].any() for c in empty[:12])


def test_ccc_sample_frame_and_empty_histogram_known_answers(oracle):
    occ = oracle.CCC(*D.load_default_model())
    img = D.sample_image()
    _, info, gains = occ.balance(img)
    assert info == [111, 139, 111, 139], info
    hist, resp = response_of(oracle, occ, img)
    flat = np.sort(resp.reshape(-1))
    assert (flat[-1] - flat[-2]) / np.spacing(flat[-1]) >= 1000
    _, info, gains = occ.balance(np.zeros_like(img))
    assert info[0:2] == [166, 106] and np.allclose(gains, [1.264, 1.0, 3.228], atol=1e-3), (info, gains)
    filt, bias = D.load_default_model()
    assert not np.array_equal(filt, filt.T) and np.unravel_index(np.argmax(bias), bias.shape) == (166, 106)
    syn = oracle.CCC(*D.model_arrays("synthetic"))
    _, info, gains = syn.balance(np.zeros_like(img))
    assert info[0:2] == [0, 0] and np.allclose(gains, [1.0, 4.145, 1.0], atol=1e-3), (info, gains)


def test_reference_model_frames_are_decided_far_above_float_noise(oracle):
    """The frames of the reference-model tests on the device: different from one another, and every arg-max at least 1000 ulp clear."""
    occ = oracle.CCC(*D.load_default_model())
    occ.set_thresholds(0.8, 0.2)
    for form, size in D.REFERENCE_MODEL_FORMS:
        frames = D.reference_model_frames(form, size, 16)
        assert len({f.tobytes() for f in frames}) == 15   # the two black frames are alike
        seen_tracks = set()
        for f in frames[:9] if form != "bgr8" else frames:
            seen = D.seen_image(oracle, form, f)
            hist, resp = response_of(oracle, occ, seen)
            flat = np.sort(resp.reshape(-1))
            assert (float(flat[-1]) - float(flat[-2])) / float(np.spacing(flat[-1])) >= 1000, (form, size)
            y, x = np.unravel_index(np.argmax(resp), resp.shape)
            seen_tracks.add((int(x), int(y)))
        assert len(seen_tracks) >= 3 and (166, 106) in seen_tracks and (111, 139) in seen_tracks, seen_tracks


# ---- the statistics kernel's headroom ---------------------------------------------------------------------------------------------
def test_headroom_geometry_and_frame(oracle):
    """launch_stats caps pairs_per_task at 128 because one wave task's sum of squares -- 64 lanes x 8 pixels x 255^2 x
    pairs_per_task -- must stay below 2^32.  1024 x 512 with stats_blocks = 8 reaches the cap, and the headroom frame fills
    every task's 32-bit sum of b^2 to within 3 % of its range."""
    w, h = D.HEADROOM_SIZE
    assert 64 * 8 * 255 ** 2 * D.MAX_PAIRS_PER_TASK < 1 << 32 <= 64 * 8 * 255 ** 2 * (D.MAX_PAIRS_PER_TASK + 2)
    for n in (1, 2):
        col_waves, pairs, n_tasks, grid_x = D.fast_stats_geometry(w, h, D.HEADROOM_STATS_BLOCKS, n)
        assert (col_waves, pairs, n_tasks, grid_x) == (4, 128, 8, 8)
    assert D.fast_stats_geometry(w, h, 2048, 1)[1] < 128   # the default budget never gets there at this size
    f = D.frame("blown_with_patch", "bayer_rggb8", w, h)
    seen = oracle.debayer(f, "bayer_rggb8")
    for ch in (0, 2):
        sums = D.task_sums(seen[..., ch], 4, 128)
        assert len(sums) == 8 and all(0.97 * 2 ** 32 < s < 2 ** 32 for s in sums), [s / 2 ** 32 for s in sums]
    # and the patch makes a wrapped sum visible in the image
    e = D.expected(oracle, "pca", {}, "bayer_rggb8", f)
    sums, mx = pca_sums(e.seen)
    assert np.array_equal(pca_apply(e.seen, pca_coeffs(sums, mx)), e.image)
    for k in (1, 3):
        s = list(sums)
        s[k] -= 1 << 32
        assert not np.array_equal(pca_apply(e.seen, pca_coeffs(s, mx)), e.image)
