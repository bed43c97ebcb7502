"""Frames with a side past 65535 and at the limits of the accepted domain: the cases of tests/test_extreme_geometry_cases.py (CPU)
and tests/test_extreme_geometry_gpu.py (PARITY.md "Geometry limits").

make_plan (rip_plan.cpp) accepts up to 2^22 pixels per side and fewer than 2^32 bytes at 3 B/px, the frame calls any row pitch
below 2^24 bytes.  Inside that domain the library takes decisions that depend on size alone -- CLAUSES below -- and a different
kernel or addressing form runs on either side of each.  A case is plain data: a size, an encoding, a stage set, a batch layout,
which clause it crosses on which side, and the kernels the clause says must (and must not) run there.  The kernel expectations are
written from the clauses, not from a run.

Importable without a GPU and without torch; nothing here looks at the library.  The functions that evaluate a case take the oracle
module as a parameter."""
import collections
import functools

import numpy as np

from helpers import cfg, expected_mht, oracle_maps, oracle_run
from raw_image_pipeline_amd import synth

SIDE_LIMIT = 1 << 22            # rip_plan.cpp make_plan
PITCH_LIMIT = 1 << 24           # rip_plan.cpp resolve_output_layout, rip_api.cpp rip_apply_device
RESIZE_LIMIT = 16384            # rip_resize.hpp kRszMaxSide, rip_area.hpp kAreaMaxSide, rip_host.cpp check_output_size
TOO_LARGE = "image too large: a frame must stay below 4 GiB and 4 Mpx per side"
PITCH_TOO_LARGE = "row pitch too large: pitches must stay below 16 MiB and a frame below 4 GiB"

SIDES = ("below", "at", "above")

# clause -> (where the code states it, what it decides, the sides a case can stand on).  "at" is the last value the near side takes.
CLAUSES = collections.OrderedDict([
    ("remap_dst_65535", ("rip_remap.hip launch_remap_tiled, rip_fused.hip launch_remap_fused: drows <= 65535 && dcols <= 65535",
                         "tiled / ring / fused remap inside, remap_vec4_kernel / remap_generic_kernel outside", SIDES)),
    ("border_list_65535", ("rip_host.cpp compile_remap_plan, rip_maps.hip remap_plan_kernel: the y << 16 | x border list",
                           "remap_border(_bayer)_kernel inside; outside the plain gather produces the border pixels itself", SIDES)),
    ("footprint_groups_65535", ("rip_batch.cpp plan_route, rip_api.cpp rip_debug_chain_footprint: cols / 4 <= 65535",
                                "the chain's item list (pair << 16 | grp) inside, the dense walk outside", SIDES)),
    ("footprint_pairs_65535", ("rip_batch.cpp plan_route, rip_api.cpp rip_debug_chain_footprint: rows / 2 <= 65535",
                               "the chain's item list (pair << 16 | grp) inside, the dense walk outside", SIDES)),
    ("chain_cols_65535", ("no clause: the chain, statistics and demosaic kernels take any width of the domain",
                          "a 16-bit column or group field anywhere in them would wrap", SIDES)),
    ("chain_rows_65535", ("no clause: the chain, statistics and demosaic kernels take any height of the domain",
                          "a 16-bit row or pair field anywhere in them would wrap", SIDES)),
    ("chain_groups_65535", ("no clause: cols / 4 against 65535 without undistortion", "as above, for the 4-pixel group index", SIDES)),
    ("chain_pairs_65535", ("no clause: rows / 2 against 65535 without undistortion", "as above, for the row-pair index", SIDES)),
    ("output_rows_65535", ("rip_output.hip launch: gridDim.y = min(rows, 65535), rows strided by gridDim.y",
                           "one trip of the row loop inside, a second trip outside", SIDES)),
    ("resize_side_16384", ("rip_host.cpp check_output_size, rip_plan.cpp apply_output_format, rip_resize.hip, rip_area.hip: every side <= 16384",
                           "resize_kernel / area_reduce_kernel inside, RIP_ERR_INVALID_ARGUMENT outside (so gridDim.y never reaches 65535 "
                           "and the area kernel's grid.y never exceeds 2048)", ("at", "above"))),
    ("side_2p22", ("rip_plan.cpp make_plan: rows, cols <= 2^22", "processed inside (ItemMap::split's largest quotient, the largest "
                   "__umul24 row index, the largest 1-D tile grids), RIP_ERR_INVALID_ARGUMENT outside", ("at", "above"))),
    ("pitch_2p24", ("rip_api.cpp rip_apply_device, rip_chain.hip chain_uses_*_path, rip_device.hpp bayer_fast_geometry: step < 2^24",
                    "processed inside (the largest __umul24 step), RIP_ERR_INVALID_ARGUMENT outside: the guards' far side is unreachable",
                    ("at", "above"))),
    # two sizings without a far side a test can afford: the second term of the statistics grids binds from 2048 * 2^16 four-pixel
    # items (sixteen colour frames of 33.5 Mpx, or one of 537 Mpx) and 2^28 pixels on; the 1-D grids stay below 2^31 everywhere
    ("stats_grid_blocks", ("rip_stats.hip launch_stats: blocks >= items >> 16 (colour), npix >> 18 (generic)",
                           "the block count of the persistent grid inside; frames large enough for the other term are not tested", ("below",))),
    ("tile_grid_1d", ("rip_demosaic.hip launch_demosaic_mht, rip_raw16_dev.hpp, rip_maps.hip launch_undistort_maps: 1-D grids of tiles / row blocks",
                      "thousands of tiles along one axis; the grids cannot pass 2^31 inside the domain", ("below",))),
    ("frame_bytes_2p32", ("rip_plan.cpp make_plan: rows * cols * 3 < 2^32", "RIP_ERR_INVALID_ARGUMENT outside, before a byte of the frame is "
                          "touched; the fast kernels' step * rows < 2^32 guards therefore never see their far side", ("above",))),
])

STAGE_SETS = {
    "debayer": dict(),
    "gamma": dict(gamma=True, gamma_k=0.8),                                                    # what a one-channel frame takes
    "memory": dict(cc=True, gamma=True, gamma_k=0.8),                                          # + the white balance of the case
    "full": dict(cc=True, gamma=True, gamma_k=0.8, vig=True, ce=True, ce_sat=1.2, ce_val=0.9),
}

Case = collections.namedtuple("Case", [
    "name", "family", "size", "encoding", "stages", "flip", "wb", "n", "layout", "method", "calib", "balance", "target", "crosses",
    "kernels", "forbidden", "extra"])


def _case(name, family, size, encoding, stages="debayer", flip=None, wb=None, n=1, layout="host", method="bilinear", calib=None,
          balance=0.0, target=None, crosses=(), kernels=(), forbidden=(), **extra):
    for clause, side in crosses:
        assert side in CLAUSES[clause][2], (name, clause, side)
    return Case(name, family, size, encoding, stages, flip, wb, n, layout, method, calib, balance, target, tuple(crosses), tuple(kernels),
                tuple(forbidden), extra)


# ---- which kernel a clause selects (rip_chain.hip chain_uses_*_path, rip_stats.hip launch_stats) ------------------------------
ALIGNED_LAYOUTS = ("host", "tight", "pitch16")   # dword-aligned base, pitch and frame stride (tight: for the widths used here)


def chain_kernel(size, encoding, flip, layout):
    """The chain kernel of an 8-bit frame without undistortion, from the geometry clauses alone."""
    w, h = size
    row = w * (3 if encoding in ("bgr8", "rgb8") else 1)
    aligned = layout in ALIGNED_LAYOUTS and (layout == "pitch16" or row % 4 == 0)
    quarter = flip in (90, 270)
    if encoding.startswith("bayer_") and aligned and w % 4 == 0 and h % 2 == 0 and w >= 4 and h >= 4:
        return "chain_rot_kernel<*>" if quarter else "chain_fast_kernel<*>"
    if encoding in ("bgr8", "rgb8") and aligned and w % 4 == 0 and not quarter:
        return "chain_color_kernel<*>"
    if encoding == "mono8" and aligned and w % 4 == 0 and not quarter:
        return "chain_mono_kernel"
    return "chain_generic_kernel"


def stats_kernel(size, encoding, layout, wb):
    w, h = size
    if wb is None or encoding == "mono8":
        return None
    if wb == "ccc":
        return "ccc_hist*kernel"
    row = w * (3 if encoding in ("bgr8", "rgb8") else 1)
    aligned = layout in ALIGNED_LAYOUTS and (layout == "pitch16" or row % 4 == 0)
    if encoding.startswith("bayer_") and aligned and w % 4 == 0 and h % 2 == 0 and w >= 4 and h >= 4:
        return "stats_fast_kernel<?>"
    if encoding in ("bgr8", "rgb8") and aligned and w % 4 == 0:
        return "stats_color_kernel"
    return "stats_generic_kernel"


CHAIN_KERNELS = ("chain_fast_kernel<*>", "chain_rot_kernel<*>", "chain_color_kernel<*>", "chain_mono_kernel", "chain_generic_kernel")
STATS_KERNELS = ("stats_fast_kernel<?>", "stats_color_kernel", "stats_generic_kernel")
TILED_REMAPS = ("remap_ring_kernel<*>", "remap_tiled_kernel<*>", "remap_bayer_ring_kernel<*>", "remap_border_kernel", "remap_border_bayer_kernel")
PLAIN_REMAPS = ("remap_vec4_kernel", "remap_generic_kernel<?>")


def _chain(name, size, encoding, stages, flip, wb, n, layout, crosses, method="bilinear", **extra):
    own_pass = method == "mht" or "range16" in extra or "packed" in extra
    if not own_pass:
        k = chain_kernel(size, encoding, flip, layout)
        kernels, forbidden = [k], [c for c in CHAIN_KERNELS if c != k]
        s = stats_kernel(size, encoding, layout, wb)
    else:   # a demosaic pass of its own (it flips as it writes) in front of the colour chain, which sees a dword-aligned bgr8 image
        kernels = ["demosaic_mht_tile_kernel<*>" if method == "mht" else "raw16_tile_kernel<%s*>" % ("StagePacked<" if "packed" in extra else "StageU16")]
        forbidden = ["chain_fast_kernel<*>", "chain_rot_kernel<*>"]
        s = stats_kernel(size[::-1] if flip in (90, 270) else size, "bgr8", "pitch16", wb)
    crosses = list(crosses)
    if s and s.startswith("stats_"):
        kernels.append(s)
        forbidden += [c for c in STATS_KERNELS if c != s]
        if s != "stats_fast_kernel<?>":
            crosses.append(("stats_grid_blocks", "below"))
    elif s:
        kernels.append(s)
    if own_pass:
        crosses.append(("tile_grid_1d", "below"))
    return _case(name, "chain", size, encoding, stages, flip, wb, n, layout, method, crosses=crosses, kernels=kernels, forbidden=forbidden, **extra)


def build_chain_cases():
    """Section 1: chain, statistics and demosaic kernels, no undistortion.  One case per clause and side, the stage sets, flips,
    white-balance methods, inputs and layouts spread over them."""
    C = _chain
    return [
        C("65532x8 rggb8 debayer host", (65532, 8), "bayer_rggb8", "debayer", None, None, 1, "host", [("chain_cols_65535", "below")]),
        C("65535x8 bgr8 memory simple", (65535, 8), "bgr8", "memory", 0, "simple", 1, "host", [("chain_cols_65535", "at")]),
        C("65536x8 grbg8 memory grey flip180 tight x3", (65536, 8), "bayer_grbg8", "memory", 180, "grey_world", 3, "tight", [("chain_cols_65535", "above")]),
        C("65536x8 rggb8 debayer base_off x3", (65536, 8), "bayer_rggb8", "debayer", None, None, 3, "base_off", [("chain_cols_65535", "above")]),
        C("65532x8 bgr8 full simple tight x3", (65532, 8), "bgr8", "full", 0, "simple", 3, "tight", [("chain_cols_65535", "below")]),
        C("65536x8 rggb8 mht full grey tight x3", (65536, 8), "bayer_rggb8", "full", 0, "grey_world", 3, "tight", [("chain_cols_65535", "above")], method="mht"),
        C("262136x4 rggb8 memory grey", (262136, 4), "bayer_rggb8", "memory", 0, "grey_world", 1, "host", [("chain_groups_65535", "below")]),
        C("262140x4 gbrg8 full pca pitch16 x3", (262140, 4), "bayer_gbrg8", "full", 0, "pca", 3, "pitch16", [("chain_groups_65535", "at")]),
        C("262140x4 mono8 gamma pitch16 x3", (262140, 4), "mono8", "gamma", 0, None, 3, "pitch16", [("chain_groups_65535", "at")]),
        C("262144x4 bggr8 memory simple flip180 host", (262144, 4), "bayer_bggr8", "memory", 180, "simple", 1, "host", [("chain_groups_65535", "above")]),
        C("262144x4 rggb16 memory grey flip180 host", (262144, 4), "bayer_rggb16", "memory", 180, "grey_world", 1, "host", [("chain_groups_65535", "above")],
          range16=(256, 60000)),
        C("262148x6 rggb8 full grey flip90 tight x3", (262148, 6), "bayer_rggb8", "full", 90, "grey_world", 3, "tight", [("chain_groups_65535", "above")]),
        C("70001x5 rggb8 memory grey flip270 host", (70001, 5), "bayer_rggb8", "memory", 270, "grey_world", 1, "host", [("chain_cols_65535", "above")]),
        C("8x65534 rggb8 debayer flip90 host", (8, 65534), "bayer_rggb8", "debayer", 90, None, 1, "host", [("chain_rows_65535", "below")]),
        C("8x65535 bgr8 memory grey tight x3", (8, 65535), "bgr8", "memory", 180, "grey_world", 3, "tight", [("chain_rows_65535", "at")]),
        C("8x65536 bgr8 memory grey flip180 base_off x3", (8, 65536), "bgr8", "memory", 180, "grey_world", 3, "base_off", [("chain_rows_65535", "above")]),
        C("8x65536 grbg8 mht memory pca flip90 host", (8, 65536), "bayer_grbg8", "memory", 90, "pca", 1, "host", [("chain_rows_65535", "above")], method="mht"),
        C("4x131068 rggb8 memory pca", (4, 131068), "bayer_rggb8", "memory", 0, "pca", 1, "host", [("chain_pairs_65535", "below")]),
        C("4x131070 mono8 gamma flip180 tight x3", (4, 131070), "mono8", "gamma", 180, None, 3, "tight", [("chain_pairs_65535", "at")]),
        C("4x131070 gbrg8 full grey flip180 tight x3", (4, 131070), "bayer_gbrg8", "full", 180, "grey_world", 3, "tight", [("chain_pairs_65535", "at")]),
        C("4x131072 rggb8 memory pca pitch16 x3", (4, 131072), "bayer_rggb8", "memory", 0, "pca", 3, "pitch16", [("chain_pairs_65535", "above")]),
        C("4x131072 rggb12p gamma host", (4, 131072), "bayer_rggb12p", "gamma", 0, None, 1, "host", [("chain_pairs_65535", "above")], packed="12p"),
        C("6x131076 rggb8 full simple flip270 host", (6, 131076), "bayer_rggb8", "full", 270, "simple", 1, "host", [("chain_pairs_65535", "above")]),
        C("5x70001 bgr8 memory simple pitch_odd x3", (5, 70001), "bgr8", "memory", 0, "simple", 3, "pitch_odd", [("chain_rows_65535", "above")]),
        # a short ccc sequence: the estimator shrinks every frame to 360 x 270, so any shape runs it; temporal consistency on
        C("65536x8 bgr8 ccc sequence x2", (65536, 8), "bgr8", "debayer", 0, "ccc", 2, "host", [("chain_cols_65535", "above")], sequence=True),
    ]


# ---- section 2: undistortion -----------------------------------------------------------------------------------------------
def camera(w, h):
    """synth.camera_model for a wide frame; for a tall one its transpose (the long axis carries the focal length either way: with
    synth.camera_model's width-scaled focal length a frame 8 pixels wide would see its whole height through a 4-pixel lens)."""
    if w >= h:
        return synth.camera_model(w, h)
    c = synth.camera_model(h, w)
    fx, cx, fy, cy = c["K"][0], c["K"][2], c["K"][4], c["K"][5]
    return dict(K=[fy, 0.0, cy, 0.0, fx, cx, 0.0, 0.0, 1.0], D=list(c["D"]), R=list(c["R"]),
                P=[fy, 0.0, cy, 0.0, 0.0, fx, cx, 0.0, 0.0, 0.0, 1.0, 0.0], width=w, height=h)


def build_undistort_cases():
    """The 65535 bound on both destination axes.  Bayer frames with the memory-rate chain in front: the fused kernel is eligible
    inside, the chain kernel followed by the plain gather run outside.  bgr8 / mono8 frames with undistortion alone are gathered as
    they lie: by the ring kernel inside (their rows 16-byte aligned: layout pitch16, or a width whose rows are), by the plain
    gather outside.  Balance 0.5: 2.3 % of the destination lies outside the source and 16 % takes the border path."""
    U = functools.partial(_case, family="undistort", balance=0.5)
    both = [("remap_dst_65535", None), ("border_list_65535", None)]

    def cross(side):
        return [(c, side) for c, _ in both]
    fused = dict(kernels=["remap_bayer_ring_kernel<*>", "remap_border_bayer_kernel"], forbidden=CHAIN_KERNELS + PLAIN_REMAPS + ("remap_ring_kernel<*>", "remap_tiled_kernel<*>"))
    two = dict(kernels=["chain_fast_kernel<*>", "remap_vec4_kernel"], forbidden=TILED_REMAPS + ("remap_generic_kernel<?>",))
    generic = dict(kernels=["chain_generic_kernel", "remap_generic_kernel<3>"], forbidden=TILED_REMAPS + ("remap_vec4_kernel",))
    ring3 = dict(kernels=["remap_ring_kernel<?, 3, false>", "remap_border_kernel"], forbidden=CHAIN_KERNELS + PLAIN_REMAPS)
    ring1 = dict(kernels=["remap_ring_kernel<?, 1, false>", "remap_border_kernel"], forbidden=CHAIN_KERNELS + PLAIN_REMAPS)
    vec4 = dict(kernels=["remap_vec4_kernel"], forbidden=CHAIN_KERNELS + TILED_REMAPS + ("remap_generic_kernel<?>",))
    gen1 = dict(kernels=["remap_generic_kernel<1>"], forbidden=CHAIN_KERNELS + TILED_REMAPS + ("remap_vec4_kernel",))
    gen3 = dict(kernels=["remap_generic_kernel<3>"], forbidden=CHAIN_KERNELS + TILED_REMAPS + ("remap_vec4_kernel",))
    m = dict(stages="memory", flip=180, wb="grey_world", n=3, layout="tight")
    m16 = dict(m, layout="pitch16")   # the fused kernel stages Bayer rows with 16-byte loads: src_step % 16 == 0 (rip_fused.hip)
    return [
        U("und 65532x8 rggb8 chain in front", size=(65532, 8), encoding="bayer_rggb8", crosses=cross("at"), host_plan=True, saturates="x", **m16, **fused),
        U("und 65536x8 rggb8 chain in front", size=(65536, 8), encoding="bayer_rggb8", crosses=cross("above"), host_plan=True, **m, **two),
        U("und 65537x8 rggb8 chain in front", size=(65537, 8), encoding="bayer_rggb8", crosses=cross("above"), **m, **generic),
        U("und 8x65534 grbg8 chain in front", size=(8, 65534), encoding="bayer_grbg8", crosses=cross("below"), host_plan=True, saturates="y", **m16, **fused),
        # an odd height: no fast Bayer geometry, so the generic chain writes the intermediate image the ring kernel gathers from
        U("und 8x65535 rggb8 chain in front", size=(8, 65535), encoding="bayer_rggb8", crosses=cross("at"), stages="memory", flip=180, wb="grey_world", n=3,
          layout="tight", kernels=["chain_generic_kernel", "remap_ring_kernel<?, 3, false>", "remap_border_kernel"],
          forbidden=PLAIN_REMAPS + ("remap_bayer_ring_kernel<*>",)),
        U("und 8x65536 rggb8 chain in front", size=(8, 65536), encoding="bayer_rggb8", crosses=cross("above"), host_plan=True, **m, **two),
        U("und 65532x8 bgr8 alone", size=(65532, 8), encoding="bgr8", n=2, layout="pitch16", crosses=cross("at"), host_plan=True, **ring3),
        U("und 65536x8 bgr8 alone", size=(65536, 8), encoding="bgr8", n=2, layout="tight", crosses=cross("above"), **vec4),
        U("und 65537x8 bgr8 alone", size=(65537, 8), encoding="bgr8", n=2, layout="tight", crosses=cross("above"), **gen3),
        U("und 8x65536 bgr8 alone", size=(8, 65536), encoding="bgr8", n=2, layout="tight", crosses=cross("above"), **vec4),
        U("und 65532x8 mono8 alone", size=(65532, 8), encoding="mono8", n=2, layout="pitch16", crosses=cross("at"), **ring1),
        U("und 65536x8 mono8 alone", size=(65536, 8), encoding="mono8", n=2, layout="tight", crosses=cross("above"), **gen1),
        U("und 8x65534 mono8 alone", size=(8, 65534), encoding="mono8", n=2, layout="pitch16", crosses=cross("below"), **ring1),
        U("und 8x65536 mono8 alone", size=(8, 65536), encoding="mono8", n=2, layout="tight", crosses=cross("above"), **gen1),
    ]


def build_footprint_cases():
    """The footprint bound, through a calibration smaller than the image: the map of a 1024 x 8 (8 x 1024) camera over a source whose
    long side is at, below and past 4 * 65535 (2 * 65535).  The full stage set keeps the chain a kernel of its own in front of the
    ring remap.  Balance 1: the map reaches column (row) 0 of the source, and with flip 180 that is the LAST group (pair) of the
    chain's input, so at the bound the list holds grp = 65534 (pair = 65534)."""
    F = functools.partial(_case, family="footprint", encoding="bayer_rggb8", stages="full", wb="grey_world", n=2, layout="tight", balance=1.0)
    listed = dict(kernels=["chain_fast_kernel<*, true>", "remap_ring_kernel<?, 3, false>"], forbidden=["chain_fast_kernel<*, false>", "chain_generic_kernel"] + list(PLAIN_REMAPS))
    dense = dict(kernels=["chain_fast_kernel<*, false>", "remap_ring_kernel<?, 3, false>"], forbidden=["chain_fast_kernel<*, true>", "chain_generic_kernel"] + list(PLAIN_REMAPS))
    return [
        F("footprint 262136x8 flip0", size=(262136, 8), flip=0, calib=(1024, 8), crosses=[("footprint_groups_65535", "below")], walk="footprint", **listed),
        F("footprint 262140x8 flip180", size=(262140, 8), flip=180, calib=(1024, 8), crosses=[("footprint_groups_65535", "at")], walk="footprint", **listed),
        F("footprint 262144x8 flip180", size=(262144, 8), flip=180, calib=(1024, 8), crosses=[("footprint_groups_65535", "above")], walk="dense", **dense),
        F("footprint 8x131068 flip180", size=(8, 131068), flip=180, calib=(8, 1024), crosses=[("footprint_pairs_65535", "below")], walk="footprint", **listed),
        F("footprint 8x131070 flip180", size=(8, 131070), flip=180, calib=(8, 1024), crosses=[("footprint_pairs_65535", "at")], walk="footprint", **listed),
        F("footprint 8x131072 flip0", size=(8, 131072), flip=0, calib=(8, 1024), crosses=[("footprint_pairs_65535", "above")], walk="dense", **dense),
    ]


# ---- section 3: delivered frames -------------------------------------------------------------------------------------------
def build_output_cases():
    """Output formats on a tall delivered frame: 4 x 65540 makes the row loop of output_convert_kernel take a second trip for rows
    0 .. 4; 65535 rows are the last single trip.  Three resident bgr8 frames, no stage; one format into a pitched destination."""
    O_ = functools.partial(_case, family="output", encoding="bgr8", n=3, layout="tight")
    out = [O_("output %s 4x65540" % f, size=(4, 65540), target=None, crosses=[("output_rows_65535", "above")], fmt=f, pitch="tight")
           for f in ("rgb8", "mono8", "rgb_chw_f32", "bgr_chw_f16")]
    out.append(O_("output rgb_chw_f32 4x65540 pitched", size=(4, 65540), crosses=[("output_rows_65535", "above")], fmt="rgb_chw_f32", pitch="pitch16"))
    out.append(O_("output rgb8 5x65535", size=(5, 65535), crosses=[("output_rows_65535", "at")], fmt="rgb8", pitch="tight"))
    out.append(O_("output bgr_chw_f16 4x65534", size=(4, 65534), crosses=[("output_rows_65535", "below")], fmt="bgr_chw_f16", pitch="tight"))
    return out


def build_resize_cases():
    """rip_set_output_size takes targets of 1 .. 16384 per side and sources up to 16384 per side (include/rip.h): the row loops of
    resize_kernel never take a second trip (gridDim.y <= 16384) and area_reduce_kernel's grid.y is at most 2048.  The sizes past
    65535 are refused before anything is enqueued; the limit itself runs."""
    R_ = functools.partial(_case, family="resize", n=2, layout="tight")
    at, above = [("resize_side_16384", "at")], [("resize_side_16384", "above")]
    return [
        R_("resize linear 16x1000 -> 8x70000 refused", size=(16, 1000), encoding="bgr8", target=(8, 70000), crosses=above, interp="linear", refused="16384"),
        R_("resize mean 6x140000 -> 3x70000 refused", size=(6, 140000), encoding="bgr8", target=(3, 70000), crosses=above, interp="linear", refused="16384"),
        R_("resize area 4x1048592 -> 2x524296 refused", size=(4, 1048592), encoding="mono8", target=(2, 524296), crosses=above, interp="area", refused="16384"),
        R_("resize area 4x1048560 -> 2x524280 refused", size=(4, 1048560), encoding="mono8", target=(2, 524280), crosses=above, interp="area", refused="16384"),
        R_("resize mean 6x32768 -> 3x16384 refused by its source", size=(6, 32768), encoding="bgr8", target=(3, 16384), crosses=above, interp="linear",
           refused="16384"),
        R_("resize linear 16x1000 -> 8x16384", size=(16, 1000), encoding="bgr8", target=(8, 16384), crosses=at, interp="linear",
           kernels=["resize_kernel<3, false>"], grid_y=16384),
        R_("resize mean 6x16384 -> 3x8192", size=(6, 16384), encoding="bgr8", target=(3, 8192), crosses=at, interp="linear",
           kernels=["resize_kernel<3, true>"], grid_y=8192),
        R_("resize area 4x16384 -> 2x8190", size=(4, 16384), encoding="mono8", target=(2, 8190), crosses=at, interp="area",
           kernels=["area_reduce_kernel<1, false>"], grid_y=1024),
    ]


# ---- section 4: the accepted limits themselves -------------------------------------------------------------------------------
def build_limit_cases():
    L = functools.partial(_case, family="limit")
    at, above = [("side_2p22", "at")], [("side_2p22", "above")]
    fast = dict(kernels=["chain_fast_kernel<*>"], forbidden=["chain_generic_kernel"])
    grey = dict(stages="gamma", flip=180, wb="grey_world")
    return [
        L("limit 8x4194304 rggb8 debayer", size=(8, SIDE_LIMIT), encoding="bayer_rggb8", n=1, layout="tight", crosses=at, **fast),
        L("limit 8x4194304 rggb8 grey gamma flip180", size=(8, SIDE_LIMIT), encoding="bayer_rggb8", n=1, layout="tight", crosses=at,
          kernels=["chain_fast_kernel<*>", "stats_fast_kernel<?>"], forbidden=["chain_generic_kernel", "stats_generic_kernel"], **grey),
        L("limit 4194304x4 grbg8 debayer", size=(SIDE_LIMIT, 4), encoding="bayer_grbg8", n=1, layout="tight", crosses=at, **fast),
        L("limit 4194304x4 grbg8 grey gamma flip180", size=(SIDE_LIMIT, 4), encoding="bayer_grbg8", n=1, layout="tight", crosses=at,
          kernels=["chain_fast_kernel<*>", "stats_fast_kernel<?>"], forbidden=["chain_generic_kernel", "stats_generic_kernel"], **grey),
        L("limit 4194305x3 refused", size=(SIDE_LIMIT + 1, 3), encoding="bayer_rggb8", crosses=above, refused=TOO_LARGE),
        L("limit 3x4194305 refused", size=(3, SIDE_LIMIT + 1), encoding="bayer_rggb8", crosses=above, refused=TOO_LARGE),
        # three rows (the generic kernels: a fast Bayer geometry has an even height) and four (the fast kernel) 2^24 - 16 bytes apart
        L("limit pitch 2^24-16 three rows", size=(64, 3), encoding="bayer_rggb8", stages="memory", wb="grey_world", n=1, layout="pitched",
          crosses=[("pitch_2p24", "at")], pitch=PITCH_LIMIT - 16, kernels=["chain_generic_kernel"], forbidden=["chain_fast_kernel<*>"]),
        L("limit pitch 2^24-16 four rows", size=(64, 4), encoding="bayer_rggb8", stages="memory", wb="grey_world", n=1, layout="pitched",
          crosses=[("pitch_2p24", "at")], pitch=PITCH_LIMIT - 16, kernels=["chain_fast_kernel<*>", "stats_fast_kernel<?>"], forbidden=["chain_generic_kernel"]),
        L("limit pitch 2^24 refused", size=(64, 3), encoding="bayer_rggb8", layout="pitched", crosses=[("pitch_2p24", "above")], pitch=PITCH_LIMIT,
          refused=PITCH_TOO_LARGE),
        # 4194304 x 342 x 3 = 4 303 355 904 >= 2^32: refused by make_plan, which rip_query_output runs before process() looks at the frame
        L("limit frame bytes 4194304x342 refused", size=(SIDE_LIMIT, 342), encoding="mono8", crosses=[("frame_bytes_2p32", "above")], refused=TOO_LARGE,
          lazy=True),
    ]


CASES = (build_chain_cases() + build_undistort_cases() + build_footprint_cases() + build_output_cases() + build_resize_cases() +
         build_limit_cases())
BY_NAME = collections.OrderedDict((c.name, c) for c in CASES)
assert len(BY_NAME) == len(CASES)


def family(name):
    return [c for c in CASES if c.family == name]


def case_id(case):
    return case.name.replace(" ", "_")


def refused(case):
    return case.extra.get("refused")


# ---- configuration and frames of a case --------------------------------------------------------------------------------------
def configuration(case):
    c = dict(STAGE_SETS[case.stages])
    if case.flip is not None:
        c.update(flip=True, flip_angle=case.flip)
    if case.wb is not None:
        c.update(wb=True, wb_method=case.wb, wb_bright=0.8, wb_dark=0.2, wb_percentile=10.0, wb_temporal=bool(case.extra.get("sequence")))
    if case.encoding == "mono8":
        c.pop("vig", None)
    if case.family in ("undistort", "footprint"):
        cw, ch = case.calib or case.size
        c.update(undistort=True, cam=camera(cw, ch), balance=case.balance)
    return cfg(**c)


def _seed(case):
    return 31000 + list(BY_NAME).index(case.name)


def _tinted_noise(w, h, seed, cn):
    """iid bytes under a tint: what the 2^22-side frames hold (a scene of 33 Mpx costs seconds and gigabytes to synthesise)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w) if cn == 1 else (h, w, cn), dtype=np.uint8)
    if cn == 1:   # a mosaic: its even columns darker, so the channel sums differ whatever the pattern
        a[:, 0::2] = (a[:, 0::2] >> 1) + 20
    else:
        a[..., 0] = (a[..., 0] >> 1) + 20
    return a


@functools.lru_cache(maxsize=8)
def _base_frame(name):
    case = BY_NAME[name]
    w, h = case.size
    enc = case.encoding
    if max(w, h) >= SIDE_LIMIT:
        return _tinted_noise(w, h, _seed(case), 1)
    if case.family in ("output", "resize"):   # every byte value in every neighbourhood: one wrong row or tap shows
        return np.random.default_rng(_seed(case)).integers(0, 256, (h, w) if enc == "mono8" else (h, w, 3), dtype=np.uint8)
    if enc in ("bgr8", "rgb8"):
        return synth.gen_scene_bgr(w, h, _seed(case), (0.62, 1.0, 0.5))
    if enc == "mono8":
        return np.ascontiguousarray(synth.gen_scene_bgr(w, h, _seed(case))[..., 1])
    pattern = enc[:10] + "8"
    return synth.gen_frame(w, h, pattern, seed=_seed(case), kind="scene", tint=(0.62, 1.0, 0.5))


def frames(case):
    """The n 8-bit frames of a case (for 16-bit and packed input: the 8-bit mosaics the samples are made of).  Frame k > 0 is frame
    0 moved by 2 k pixels along the long axis, darkened and lifted: a different image with different white-balance sums whose Bayer
    phase is the same."""
    base = _base_frame(case.name)
    axis = 1 if case.size[0] >= case.size[1] else 0
    out = [base]
    for k in range(1, case.n):
        f = np.roll(base, 2 * k, axis=axis).astype(np.uint16) * (5 - k) // 5 + 11 * k
        if f.ndim == 3:
            f[..., 2] = f[..., 2] * (4 + k) // 6
        out.append(f.astype(np.uint8))
    for f in out:
        f.setflags(write=False)
    return out


def samples16(case, frame8):
    """uint16 samples of a 16-bit or packed case from its 8-bit mosaic."""
    if "packed" in case.extra:
        return (frame8.astype(np.uint16) << 4) | (frame8.astype(np.uint16) >> 4)          # 12 bits, every low nibble used
    black, white = case.extra["range16"]
    return (black + frame8.astype(np.uint32) * (white - black + 700) // 255).clip(0, 65535).astype(np.uint16)   # a little past white


def range16(case):
    return (0, 4095) if "packed" in case.extra else case.extra["range16"]


# ---- the oracle's answer --------------------------------------------------------------------------------------------------
def expected_images(O, case):
    """The oracle's image of every frame of a case, before any output stage (format, resize)."""
    from raw16_reference import expected_raw16
    c = configuration(case)
    fs = frames(case)
    if case.extra.get("sequence"):
        filt, bias = synth.ccc_model()
        occ = O.CCC(filt, bias)
        occ.set_kalman_model(1.0, 10.0)
        occ.set_thresholds(0.8, 0.2)
        occ.set_temporal_consistency(True)
        return [oracle_run(O, c, np.ascontiguousarray(f), case.encoding, ccc=occ)[0] for f in fs]
    if "range16" in case.extra or "packed" in case.extra:
        black, white = range16(case)
        return [expected_raw16(O, c, samples16(case, f), case.encoding[:10] + "16", case.method, black, white)[0] for f in fs]
    if case.method == "mht":
        return [expected_mht(O, c, np.ascontiguousarray(f), case.encoding)[0] for f in fs]
    return [oracle_run(O, c, np.ascontiguousarray(f), case.encoding)[0] for f in fs]


def delivered(O, case, images):
    """What the handle delivers for the oracle's images of an output or resize case."""
    import area_reference
    import output_reference
    import output_variant_cases
    import resize_reference
    if case.family == "output":
        return [output_reference.convert(e, case.extra["fmt"], *output_variant_cases.NORM) for e in images]
    tw, th = case.target
    if case.extra["interp"] == "area":
        return [area_reference.resize(e, th, tw) for e in images]
    return [resize_reference.resize(e, th, tw) for e in images]


def saturated_fraction(O, case):
    """The share of destination pixels whose integer source coordinate cv::remap saturates to 32767 (rip_remap_dev.hpp,
    the oracle's sat_s16_i) along the axis the case names."""
    mx, my = oracle_maps(O, configuration(case))
    m = mx if case.extra["saturates"] == "x" else my
    q = np.rint(m.astype(np.float32) * np.float32(32.0)).astype(np.int64) >> 5
    return float((q > 32767).mean())


def white_balance_estimate(O, case, frame):
    """The oracle's estimate for one frame of a white-balance case, as wb_degenerate_cases.expected gives it."""
    import wb_degenerate_cases as D
    params = dict(wb_bright=0.8, wb_percentile=10.0)
    if case.method == "mht":
        from mht_reference import mht_reference
        seen = mht_reference(np.ascontiguousarray(frame), case.encoding)
        return D.expected(O, case.wb, params, "bgr8", seen).estimate
    if "range16" in case.extra:
        from raw16_reference import demosaic16, narrow16
        seen = narrow16(demosaic16(O, samples16(case, frame), case.encoding, "bilinear"), *range16(case))
        return D.expected(O, case.wb, params, "bgr8", seen).estimate
    return D.expected(O, case.wb, params, case.encoding, np.ascontiguousarray(frame)).estimate
