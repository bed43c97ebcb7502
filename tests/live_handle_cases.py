"""Model-based fuzz of ONE live handle (PARITY.md "Live handle"): a random walk of single setter calls and frame calls, a plain
dict of the settings kept beside the handle, and after every frame call the CPU expectation of the model as it then stands.

``walk(seed)`` returns the steps, pure data that prints and replays (``walk_from``):

    ("init",)                              the fixed first step: ``apply_model(pipe, initial_model())``; never again afterwards
    ("mut", setter, args, note)            ONE setter of RawImagePipeline with its arguments; note: "", "revert", "same", "double", "double revert"
    ("call", {...})                        a frame call: input kind, size, n, entry point, seeds, requested heads, getters that follow,
                                           and -- for a call the rules of include/rip.h refuse -- the expected status and message prefix

``Evaluator(oracle).replay(steps)`` yields what every accepted call must deliver, composed from the existing references only:
helpers.oracle_run / expected_mht, raw16_reference.expected_raw16, packed_reference.unpack for F and the taps; fit_reference.geometry,
resize_reference / area_reference / aa_reference, fit_reference.pad_bytes and output_reference.convert for every head; mask_cases for
the masks; wb_degenerate_cases.expected on the oracle's debayered tap for the estimates the getters expose.

The ccc estimator.  The handle has ONE filter state whatever model is loaded; the oracle has one object per model.  The rules of
include/rip.h and rip_api.cpp are mirrored: a reset only arms when the method is "ccc" at the time of the call, the covariance survives
a reset, a refused call advances nothing.  The header is silent about what a model swap does to the filter state, so a swap is only
drawn while the method is "ccc" and is always followed by a reset step, on both sides.  What survives a reset is the covariance, which
does not depend on the data: every oracle object (one per model, and a twin of each that yields the track and the gains) sees every
ccc frame, so all of them carry the covariance the handle carries.

Refusals are decided on the CPU with a ``device=-1`` probe handle that receives every mutation of the walk, and ``query_output`` under
every requested head; the two rules of the heads calls on a bgr16 result (one head, no taps) are stated here.

The generator needs the built library (the probe) but neither a GPU nor torch; the evaluator needs the CPU oracle."""
import collections
import functools

import numpy as np

import aa_reference as AA
import fit_reference as FR
import heads_cases as HC
import helpers as H
import mask_cases as MC
import mht_reference as MF
import output_reference as R
import packed_reference as PKR
import pinhole_reference as PR
import raw16_cases as G
import wb_degenerate_cases as D
from raw16_reference import demosaic16, expected_raw16, narrow16
from raw_image_pipeline_amd import synth

SEED_BASE = 52000
DEFAULT_SEEDS = tuple(range(16))
DEFAULT_STEPS = 40

# ---- what is drawn ----------------------------------------------------------------------------------------------------------------
GEOMETRIES = ((64, 48), (51, 33), (136, 72))                     # fast paths; every form on the generic kernels; no multiple of 16 per row
CAM_GEOMETRIES = ((328, 200), (320, 240), (200, 200))            # each with its camera; 200 x 200: a quarter turn keeps the plan's key
CCC_GEOMETRIES = ((384, 240), (720, 540))                        # bilinear, and the exact 2 x 2 shrink to 360 x 270
BATCHES = (1, 2, 3, 8, 9, 13, 17)
BAYER8 = ("bayer_rggb8", "bayer_bggr8", "bayer_gbrg8", "bayer_grbg8")
COLOUR = ("bgr8", "rgb8", "mono8")
BAYER16 = tuple("bayer_%s16" % n for n in G.NAMES)
PACKED = ("bayer_rggb10p", "bayer_grbg12p", "bayer_bggr10_csi2", "bayer_gbrg12_csi2")     # one packed form of each layout
INPUT_KINDS = BAYER8 + COLOUR + BAYER16 + PACKED
ENTRIES = ("process", "apply_device", "apply_device_strided", "apply_device_heads", "apply_heads", "submit_collect")
HOST_ENTRIES = ("process", "apply_heads", "submit_collect")
RING_DEPTH = 3
INTERPOLATIONS = ("linear", "area", "linear_aa", "cubic_aa")
FITS = FR.FITS
FORMATS = ("native",) + R.FORMATS
MAX_HEADS = 4
PLUMB_BOB_D = PR.CALIBRATIONS["barrel"][1]
REFUSAL_CLASSES = ("area_upscale", "aa_factor", "roi_outside", "format_on_mono", "bgr16_format", "bgr16_heads", "bgr16_tap")
RIP_ERR_INVALID_ARGUMENT, RIP_ERR_ASSERT = 1, 2

OTHER_MATRIX = (1.5, -0.2, 0.1, 0.05, 1.1, -0.1, -0.3, 0.2, 1.8)
NORMS = (R.DEFAULT_NORM, (57.0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), (128.0, (0.25, 0.5, 0.75), (0.5, 2.0, 1.5)))
ROIS = ((0, 0, 0, 0), (8, 4, 24, 20), (1, 1, 30, 19), (2, 3, 17, 25))      # every one lies inside the smallest F (33 x 33 of 51 x 33 turned)
SIZES = ((0, 0), (32, 24), (40, 30), (21, 17), (96, 64), (300, 100), (68, 36), (164, 100), (192, 120), (100, 100))   # some are halves of a geometry
PADS = ((114, 114, 114), (3, 128, 250), (0, 255, 7))

# setter -> (model key, values): getattr(pipe, setter)(value)
SCALAR = collections.OrderedDict([
    ("set_flip", ("flip", (False, True))),
    ("set_flip_angle", ("flip_angle", (0, 90, 180, 270))),
    ("set_white_balance", ("wb", (False, True))),
    ("set_white_balance_method", ("wb_method", ("grey_world", "pca", "simple", "ccc"))),
    ("set_white_balance_percentile", ("wb_percentile", (10.0, 1.0, 50.0))),
    ("set_white_balance_temporal_consistency", ("wb_temporal", (False, True))),
    ("set_color_calibration", ("cc", (False, True))),
    ("set_gamma_correction", ("gamma", (False, True))),
    ("set_gamma_correction_method", ("gamma_method", ("custom", "default"))),
    ("set_gamma_correction_k", ("gamma_k", (0.8, 2.2, 0.45))),
    ("set_vignetting_correction", ("vig", (False, True))),
    ("set_color_enhancer", ("ce", (False, True))),
    ("set_color_enhancer_hue_gain", ("ce_hue", (1.0, 1.3, 0.8))),
    ("set_color_enhancer_saturation_gain", ("ce_sat", (1.0, 0.7, 1.2))),
    ("set_color_enhancer_value_gain", ("ce_val", (1.0, 1.1, 0.9))),
    ("set_undistortion", ("undistort", (False, True))),
    ("set_undistortion_balance", ("balance", (0.0, 1.0, 0.5))),
    ("set_undistortion_fov_scale", ("fov_scale", (1.0, 0.8, 1.3))),
    ("set_fp_contraction", ("fp_contract", (0, 1))),
    ("set_debayer_method", ("debayer_method", ("bilinear", "mht"))),
    ("set_debayer_16bit", ("debayer_16bit", (False, True))),
    ("set_rect_mask", ("rect_mask", ("off", "coverage", "valid"))),
    ("set_color_calibration_matrix", ("cc_matrix", (tuple(synth.COLOR_MATRIX), OTHER_MATRIX))),
    ("set_color_calibration_bias", ("cc_bias", ((0.0, 0.0, 0.0), (3.0, -2.0, 1.5)))),
])
# setter -> (model key, values): getattr(pipe, setter)(*value)
SPREAD = collections.OrderedDict([
    ("set_white_balance_saturation_threshold", (("wb_bright", "wb_dark"), ((0.8, 0.2), (0.9, 0.1), (0.5, 0.3)))),
    ("set_vignetting_correction_parameters", ("vig_params", ((1.5, 1e-3, 1e-6), (1.2, 2e-3, 3e-6)))),
    ("set_debayer_16bit_range", ("range16", ((0, 0), (64, 1023), (0, 65535)))),
    ("set_ccc_kalman_model", ("kalman", ((1.0, 10.0), (0.0, 1.0), (1.0, 2.0)))),
])
# setter -> (field of the selected head, values, spread)
HEAD = collections.OrderedDict([
    ("set_output_format", ("format", FORMATS, False)),
    ("set_output_normalization", ("norm", NORMS, True)),
    ("set_output_size", ("size", SIZES, True)),
    ("set_output_interpolation", ("interp", INTERPOLATIONS, False)),
    ("set_output_roi", ("roi", ROIS, True)),
    ("set_output_fit", ("fit", FITS, False)),
    ("set_output_pad", ("pad", PADS, True)),
])
# only at values the suite already runs them at; the first is the library's default where the suite says so
TUNABLES = collections.OrderedDict([
    ("chain_footprint", (1, 0)), ("remap_fused", (1, 0)), ("remap_ring", (1, 0)), ("remap_stages", (3, 2, 4)), ("ccc_lds_hist_min", (12, 1, 1000000)),
    ("overlap_groups", (0, 2, 3)), ("stats_blocks", (2048, 8)), ("chain_blocks", (0, 8)), ("remap_frames", (0, 1, 4)),
])
SPECIAL = ("set_output_heads", "select_output_head", "load_camera", "set_ccc_model", "reset_white_balance_temporal_consistency", "set_tunable", "set_stream")
MUTATION_KINDS = tuple(SCALAR) + tuple(SPREAD) + tuple(HEAD) + SPECIAL

# ---- the cache table: one row per device constant or tracked buffer of rip_handle.hpp ------------------------------------------------
# stale: the mutation or call kinds after which the cache must not be used as it is.  keep: kinds that touch the same memory or the same
# settings and must NOT cost (or spoil) the cache.  Call kinds: "call:geometry" a frame size other than the previous call's,
# "call:larger" more bytes per batch than any call before (DevBuf::reserve reallocates), "call:stats" grey-world / pca statistics,
# "call:simple" SimpleWB, "call:ccc1" a single-frame ccc call (the global-atomic histogram, handed back zeroed), "call:cccN" a ccc batch.
Row = collections.namedtuple("Row", ["stale", "keep"])
CACHES = collections.OrderedDict([
    ("tables", Row(("set_gamma_correction", "set_gamma_correction_k"), ("set_gamma_correction_method", "set_color_calibration_matrix", "set_color_calibration_bias"))),
    ("vignette", Row(("set_vignetting_correction_parameters", "set_fp_contraction", "call:geometry"), ("set_vignetting_correction", "set_flip_angle"))),
    ("maps", Row(("set_undistortion_balance", "set_undistortion_fov_scale", "load_camera"), ("set_undistortion", "set_rect_mask"))),
    ("plan", Row(("set_undistortion_balance", "set_undistortion_fov_scale", "load_camera"), ("set_tunable", "set_flip"))),
    ("plan.items", Row(("set_flip_angle", "set_undistortion_balance", "load_camera"), ("set_tunable", "set_gamma_correction"))),
    ("ccc.model", Row(("set_ccc_model",), ("set_white_balance_method", "set_white_balance_saturation_threshold"))),
    ("ccc.state", Row(("set_ccc_kalman_model", "set_white_balance_temporal_consistency", "reset_white_balance_temporal_consistency"),
                      ("set_white_balance", "set_white_balance_method"))),
    ("ccc.geom", Row(("call:geometry",), ("set_flip",))),
    # set_output_heads marks the tables of the heads it resets, whose format is then "native": the next planar format marks them again
    ("out_table[k]", Row(("set_output_format", "set_output_normalization"), ("set_output_heads", "select_output_head", "set_output_size", "set_output_pad"))),
    ("rsz_tables[k]", Row(("set_output_size", "set_output_interpolation", "set_output_roi", "set_output_fit", "call:geometry"),
                          ("set_output_pad", "set_output_format", "select_output_head"))),
    ("mask_base", Row(("set_undistortion_balance", "set_undistortion_fov_scale", "load_camera", "set_undistortion", "call:geometry"), ("set_rect_mask", "select_output_head"))),
    # rip_api.cpp drops the head's mask in EVERY output setter of the head, set_output_pad / _format / _normalization included; a mask is
    # composed with pad 0, format native and no table, so no byte of it depends on those three and they cannot stand under `stale`
    # (a staling kind needs a witness whose bytes differ).  keep: what must leave the selected head's mask alone.
    ("mask_head[k]", Row(("set_output_size", "set_output_interpolation", "set_output_roi", "set_output_fit", "set_rect_mask", "set_undistortion_balance"),
                         ("select_output_head", "set_stream", "set_gamma_correction"))),
    ("d_stats.clean_bytes", Row(("call:larger", "call:simple"), ("call:ccc1", "set_white_balance_method", "set_white_balance_saturation_threshold"))),
    ("d_hist.clean_bytes", Row(("call:simple", "call:cccN"), ("call:stats", "set_white_balance_method", "set_white_balance_percentile"))),
    ("d_mid.cap", Row(("call:larger",), ("set_tunable", "set_undistortion_fov_scale"))),
    ("d_mht.cap", Row(("call:larger",), ("set_debayer_method",))),
    ("d_fmt.cap", Row(("call:larger",), ("set_output_format",))),
    ("d_rsz.cap", Row(("call:larger",), ("set_output_size",))),
])

PAIRS = [(name, kind) for name, row in CACHES.items() for kind in row.stale]

# themes: what a walk leans towards (seed % len(THEMES)), so that fill -> change -> read runs of every cache row happen within 40 steps
Theme = collections.namedtuple("Theme", ["name", "start", "boost", "kinds", "geometries", "entries"])
THEMES = (
    Theme("tables", (("set_gamma_correction", (True,)), ("set_color_calibration", (True,))),
          ("set_gamma_correction", "set_gamma_correction_k", "set_gamma_correction_method", "set_color_calibration_matrix", "set_color_calibration_bias", "set_color_enhancer",
           "set_color_enhancer_hue_gain", "set_color_enhancer_saturation_gain", "set_color_enhancer_value_gain"), BAYER8 + ("bgr8", "rgb8"), GEOMETRIES, ENTRIES),
    Theme("vignette", (("set_vignetting_correction", (True,)), ("set_gamma_correction", (True,))),
          ("set_vignetting_correction_parameters", "set_fp_contraction", "set_vignetting_correction", "set_flip_angle", "set_flip", "set_debayer_method"), BAYER8 + ("bgr8",),
          GEOMETRIES, ENTRIES),
    Theme("undistort", (("load_camera", ("equidistant", 328, 200)), ("set_undistortion", (True,)), ("set_gamma_correction", (True,))),
          ("set_undistortion_balance", "set_undistortion_fov_scale", "load_camera", "set_undistortion", "set_flip_angle", "set_flip", "set_tunable", "set_stream"), BAYER8 + ("bgr8", "mono8"),
          CAM_GEOMETRIES, ENTRIES),
    Theme("ccc", (("set_white_balance", (True,)), ("set_white_balance_method", ("ccc",)), ("set_gamma_correction", (True,))),
          ("set_ccc_model", "set_ccc_kalman_model", "set_white_balance_temporal_consistency", "reset_white_balance_temporal_consistency", "set_white_balance_saturation_threshold",
           "set_tunable", "set_flip"), BAYER8 + ("bgr8",), CCC_GEOMETRIES, ("process", "apply_device", "apply_device", "apply_device_strided")),
    Theme("heads", (("set_output_heads", (3,)), ("set_gamma_correction", (True,))),
          tuple(HEAD) + ("set_output_heads", "select_output_head", "select_output_head"), BAYER8 + COLOUR, GEOMETRIES, ("apply_device_heads", "apply_heads", "apply_device", "process")),
    Theme("masks", (("load_camera", ("equidistant", 200, 200)), ("set_undistortion", (True,)), ("set_rect_mask", ("coverage",)), ("set_output_heads", (2,))),
          ("set_rect_mask", "set_undistortion_balance", "set_undistortion_fov_scale", "load_camera", "set_undistortion", "select_output_head", "set_output_size", "set_output_interpolation",
           "set_output_roi", "set_output_fit", "set_output_pad", "set_output_format", "set_output_normalization"), BAYER8 + ("mono8", "bgr8"), CAM_GEOMETRIES, ENTRIES),
    Theme("stats", (("set_white_balance", (True,)),),
          ("set_white_balance_method", "set_white_balance_method", "set_white_balance_percentile", "set_white_balance_saturation_threshold", "set_white_balance", "set_tunable",
           "set_stream"), BAYER8 + ("bgr8", "rgb8"), GEOMETRIES + CCC_GEOMETRIES[:1], ("process", "apply_device", "apply_device_strided", "submit_collect")),
    Theme("raw16", (("set_debayer_16bit", (True,)),),
          ("set_debayer_16bit", "set_debayer_16bit_range", "set_debayer_method", "set_flip", "set_flip_angle", "set_output_format", "set_output_heads"), BAYER16 + PACKED + BAYER16, GEOMETRIES,
          ENTRIES),
)


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def initial_model():
    m = H.cfg()
    m["cc_matrix"] = tuple(m["cc_matrix"])
    m.update(debayer_method="bilinear", debayer_16bit=False, range16=(0, 0), fp_contract=0, ccc_model="synthetic", kalman=(1.0, 10.0),
             n_heads=1, selected=0, heads=(HC.DEFAULT,) * MAX_HEADS, rect_mask="off", stream=0,
             tunables=tuple((k, v[0]) for k, v in TUNABLES.items()))
    return m


def camera(cam):
    """The camera dict of a model's cam entry (model, width, height)."""
    model, w, h = cam
    return synth.camera_model(w, h) if model == "equidistant" else synth.pinhole_camera_model(w, h, PLUMB_BOB_D)


def cfg_of(m):
    """helpers.cfg of a model; a plumb_bob camera is left out (helpers.oracle_maps builds fisheye maps): see Evaluator._maps."""
    c = {k: m[k] for k in H.DEFAULTS}
    c["cc_matrix"] = list(m["cc_matrix"])
    c["cam"] = camera(m["cam"]) if m["cam"] is not None and m["cam"][0] == "equidistant" else None
    return c


def current_args(m, setter):
    """The arguments with which `setter` sets what the model already holds."""
    if setter in SCALAR:
        return (m[SCALAR[setter][0]],)
    if setter in SPREAD:
        key = SPREAD[setter][0]
        return tuple(m[k] for k in key) if isinstance(key, tuple) else tuple(m[key])
    if setter in HEAD:
        field, _, spread = HEAD[setter]
        v = getattr(m["heads"][m["selected"]], field)
        return tuple(v) if spread else (v,)
    return {"set_output_heads": (m["n_heads"],), "select_output_head": (m["selected"],), "load_camera": m["cam"], "set_ccc_model": (m["ccc_model"],),
            "reset_white_balance_temporal_consistency": (), "set_stream": (m["stream"],)}[setter]


def update_model(m, setter, args):
    """The model after `setter(*args)`; the ccc filter state lives in the Evaluator."""
    m = dict(m)
    if setter in SCALAR:
        m[SCALAR[setter][0]] = args[0]
    elif setter in SPREAD:
        key = SPREAD[setter][0]
        if isinstance(key, tuple):
            m.update(zip(key, args))
        else:
            m[key] = tuple(args)
    elif setter in HEAD:
        field, _, spread = HEAD[setter]
        heads = list(m["heads"])
        heads[m["selected"]] = heads[m["selected"]]._replace(**{field: tuple(args) if spread else args[0]})
        m["heads"] = tuple(heads)
    elif setter == "set_output_heads":
        m["n_heads"] = args[0]
        m["heads"] = tuple(h if k < args[0] else HC.DEFAULT for k, h in enumerate(m["heads"]))
        if m["selected"] >= args[0]:
            m["selected"] = 0
    elif setter == "select_output_head":
        m["selected"] = args[0]
    elif setter == "load_camera":
        m["cam"] = tuple(args)
    elif setter == "set_ccc_model":
        m["ccc_model"] = args[0]
    elif setter == "set_tunable":
        m["tunables"] = tuple((k, args[1] if k == args[0] else v) for k, v in m["tunables"])
    elif setter == "set_stream":
        m["stream"] = args[0]
    else:
        assert setter == "reset_white_balance_temporal_consistency", setter
    return m


def apply_mutation(pipe, setter, args, streams=None):
    """The ONE call on a handle that a mutation step stands for.  streams: the test's streams (index 0 is the null stream); a probe has none."""
    if setter == "load_camera":
        synth.load_camera(pipe, camera(args), args[0])
    elif setter == "set_ccc_model":
        pipe.set_ccc_model(*D.model_arrays(args[0]))
    elif setter == "set_stream":
        if streams is not None:
            pipe.set_stream(streams[args[0]])
    elif setter == "set_tunable":
        if streams is not None:          # launch tunables mean nothing to a handle without a device
            pipe.set_tunable(*args)
    elif setter in ("set_color_calibration_matrix", "set_color_calibration_bias"):
        getattr(pipe, setter)(list(args[0]))
    else:
        getattr(pipe, setter)(*args)


def apply_model(pipe, m, streams=None):
    """Step 0: every setting of the model through its setter (helpers.configure for the keys of helpers.cfg)."""
    c = cfg_of(m)
    H.configure(pipe, c)
    if m["cam"] is not None and c["cam"] is None:
        apply_mutation(pipe, "load_camera", m["cam"])
    pipe.set_undistortion_balance(m["balance"])          # helpers.configure sets them with a camera only; a new handle's are not the model's
    pipe.set_undistortion_fov_scale(m["fov_scale"])
    for setter in ("set_debayer_method", "set_debayer_16bit", "set_debayer_16bit_range", "set_fp_contraction", "set_ccc_model", "set_ccc_kalman_model", "set_rect_mask"):
        apply_mutation(pipe, setter, current_args(m, setter), streams)
    pipe.set_output_heads(m["n_heads"])
    for k in range(m["n_heads"]):
        pipe.select_output_head(k)
        HC.apply_head(pipe, m["heads"][k])
    pipe.select_output_head(m["selected"])
    if streams is not None:
        for name, value in m["tunables"]:
            pipe.set_tunable(name, value)
        pipe.set_stream(streams[m["stream"]])


# ---- what a call is, given the model ---------------------------------------------------------------------------------------------------
def input_form(kind):
    """(channels handed to the C ABI, result channels, packed layout or None, 16-bit samples)."""
    if kind in ("bgr8", "rgb8"):
        return 3, 3, None, False
    if kind == "mono8":
        return 1, 1, None, False
    layout = kind[10:] if kind[10:] in PKR.LAYOUTS else None
    return 1, 3, layout, kind.endswith("16")


def effective_flip(m):
    return m["flip_angle"] if m["flip"] and m["flip_angle"] in (90, 180, 270) else 0


def is_bgr16(m, kind):
    return kind in BAYER16 and m["range16"] == (0, 0)


def remapped(m):
    return bool(m["undistort"] and m["cam"] is not None)


def wb_mode(m, kind):
    return m["wb_method"] if m["wb"] and kind != "mono8" and not is_bgr16(m, kind) else None


def frame_count(call):
    """The frames a call processes: the host entry points take one frame per call of the C ABI, the ring holds RING_DEPTH."""
    return min(call["n"], RING_DEPTH) if call["entry"] in HOST_ENTRIES else call["n"]


def delivered_heads(m, call):
    return list(call["heads"]) if call["entry"] in ("apply_device_heads", "apply_heads") else [m["selected"]]


def head_resizes(head):
    return head.size != (0, 0) or head.roi != (0, 0, 0, 0)


def call_rows(m, call):
    """The rows of CACHES an accepted call reads (and fills)."""
    kind = call["kind"]
    rows = set()
    if is_bgr16(m, kind):
        return rows
    three = kind != "mono8"
    if m["gamma"]:
        rows.add("tables")
    if m["vig"] and three:
        rows.add("vignette")
    if remapped(m):
        rows |= {"maps", "plan", "d_mid.cap"}
        if dict(m["tunables"])["chain_footprint"] and kind in BAYER8:
            rows.add("plan.items")
    mode = wb_mode(m, kind)
    if mode == "ccc":
        rows |= {"ccc.model", "ccc.state", "ccc.geom", "d_hist.clean_bytes"}
    elif mode == "simple":
        rows |= {"d_stats.clean_bytes", "d_hist.clean_bytes"}
    elif mode is not None:
        rows.add("d_stats.clean_bytes")
    if m["debayer_method"] == "mht" and kind in BAYER8:
        rows.add("d_mht.cap")
    for k in delivered_heads(m, call):
        head = m["heads"][k]
        if three and head.format in R.TABLE_FORMATS:
            rows.add("out_table[k]")
        if head_resizes(head):
            rows.add("rsz_tables[k]")
        if three and head.format != "native":
            rows.add("d_fmt.cap")
            if head_resizes(head):
                rows.add("d_rsz.cap")
    if "rect_mask" in call["after"]:
        rows.add("mask_base")
    if "output_mask" in call["after"]:
        rows |= {"mask_base", "mask_head[k]"}
    return rows


def call_bytes(call):
    w, h = call["size"]
    return w * h * frame_count(call)


def annotate(steps):
    """[(step, model after the step, kinds, rows)]: kinds -- the setter of a mutation, the call kinds of an accepted call (see CACHES);
    rows -- the rows of CACHES an accepted call reads."""
    m, out, prev_size, largest = None, [], None, 0
    for step in steps:
        kinds, rows = set(), set()
        if step[0] == "init":
            m = initial_model()
        elif step[0] == "mut":
            m = update_model(m, step[1], step[2])
            kinds.add(step[1])
        else:
            call = step[1]
            if call["refusal"] is None:
                rows = call_rows(m, call)
                if prev_size is not None and call["size"] != prev_size:
                    kinds.add("call:geometry")
                if largest and call_bytes(call) > largest:
                    kinds.add("call:larger")
                mode = wb_mode(m, call["kind"])
                if mode in ("grey_world", "pca"):
                    kinds.add("call:stats")
                elif mode == "simple":
                    kinds.add("call:simple")
                elif mode == "ccc":
                    kinds.add("call:ccc1" if frame_count(call) == 1 or call["entry"] in HOST_ENTRIES else "call:cccN")
                prev_size, largest = call["size"], max(largest, call_bytes(call))
        out.append((step, m, kinds, rows))
    return out


def rows_of_mutation(setter):
    return [name for name, row in CACHES.items() if setter in row.stale or setter in row.keep]


# ---- the generator ---------------------------------------------------------------------------------------------------------------------
def new_probe():
    from raw_image_pipeline_amd import RawImagePipeline
    probe = RawImagePipeline(False, "", "", "", device=-1)
    apply_model(probe, initial_model())
    return probe


def probe_refusal(probe, m, call):
    """None, or the refusal of `call` under the probe's settings (the model's): dict(status, prefix, cls, message)."""
    from raw_image_pipeline_amd.pipeline import RipAssertError
    w, h = call["size"]
    cn = input_form(call["kind"])[0]
    heads_call = call["entry"] in ("apply_device_heads", "apply_heads")
    found = None
    for k in delivered_heads(m, call):
        probe.select_output_head(k)
        try:
            probe.query_output(h, w, cn, call["kind"])
        except (ValueError, RipAssertError) as e:
            msg = str(e)
            cls = "other"
            for needle, name in (("enlarges an axis", "area_upscale"), ("factors up to 64", "aa_factor"), ("does not lie inside", "roi_outside"),
                                 ("three-channel pipeline result", "format_on_mono"), ("this frame gives bgr16", "bgr16_format"),
                                 ("factors up to 256", "area_factor")):
                if needle in msg:
                    cls = name
            status = RIP_ERR_ASSERT if isinstance(e, RipAssertError) else RIP_ERR_INVALID_ARGUMENT
            # the single-output calls name no head: for them the prefix is empty and only the status is pinned
            found = dict(status=status, prefix=("output head %d: " % k) if heads_call else "", cls=cls, message=msg, head=k)
            break
    probe.select_output_head(m["selected"])
    if found is None and heads_call and is_bgr16(m, call["kind"]):
        if len(call["heads"]) > 1:
            found = dict(status=RIP_ERR_INVALID_ARGUMENT, prefix="16-bit Bayer frames without a 16-bit range give bgr16", cls="bgr16_heads", message="", head=None)
        elif call["taps"]:
            found = dict(status=RIP_ERR_INVALID_ARGUMENT, prefix="16-bit Bayer frames have no taps", cls="bgr16_tap", message="", head=None)
    return found


class Walker:
    def __init__(self, seed, n_steps):
        self.seed, self.n_steps = seed, n_steps
        self.rng = np.random.default_rng(SEED_BASE + seed)
        self.theme = THEMES[seed % len(THEMES)]
        self.m = initial_model()
        self.probe = new_probe()
        self.steps = [("init",)]
        self.prev = None            # (setter, the arguments that undo it, the head it addressed)
        self.calls = self.refusals = 0
        self.plumb_bob_used = False
        self.call_serial = self.tunable_serial = 0
        self.turn = {}
        # what this walk must draw whatever the dice say, so that the default walks together draw every kind of everything
        r = seed % len(DEFAULT_SEEDS)
        kinds = BAYER8 + COLOUR + PACKED + (BAYER16[r % 4],)
        sizes = GEOMETRIES + CAM_GEOMETRIES + CCC_GEOMETRIES
        self.must_mutate = [k for i, k in enumerate(MUTATION_KINDS) if i % len(DEFAULT_SEEDS) == r]
        listed = [(k, SCALAR[k][1] if k in SCALAR else SPREAD[k][1]) for k in ("set_white_balance_method", "set_fp_contraction", "set_debayer_method", "set_debayer_16bit_range",
                                                                                   "set_rect_mask", "set_flip_angle")]
        values = [(k, v if k in SPREAD else (v,)) for k, vs in listed for v in vs]
        self.must_mutate += [kv for i, kv in enumerate(values) if i % len(DEFAULT_SEEDS) == r]
        self.must_mutate += [("set_stream", (0,))] * (r % 3 == 0) + [("set_stream", (1 + r % 2,))]       # popped from the end: a stream of the test's first
        self.must_mutate += [("set_tunable", (name, values[1 + r % (len(values) - 1)])) for i, (name, values) in enumerate(TUNABLES.items()) if i % len(DEFAULT_SEEDS) == r]
        self.must_call = [dict(kind=kinds[r % len(kinds)]), dict(entry=ENTRIES[r % len(ENTRIES)]), dict(n=BATCHES[r % len(BATCHES)], size=GEOMETRIES[0]),
                          dict(size=sizes[r % len(sizes)]), dict(entry="apply_device_strided", layout=H.LAYOUTS[1:][r % 4], kind=BAYER8[r % 4])]

    def pick(self, values, key=None):
        """One of `values`: each list is gone through in turn, from an offset of the walk's own, so that a few walks of a few steps
        draw every value of every list; what is random is when which list is asked."""
        values = list(values)
        key = key or repr(values)
        if key not in self.turn:
            self.turn[key] = self.seed * 11 + len(key)
        self.turn[key] += 1
        return values[self.turn[key] % len(values)]

    # -- mutations
    def emit(self, setter, args, note=""):
        args = tuple(args)
        before = current_args(self.m, setter) if setter != "set_tunable" else (args[0], dict(self.m["tunables"])[args[0]])
        self.steps.append(("mut", setter, args, note))
        apply_mutation(self.probe, setter, args)
        head = self.m["selected"]
        self.m = update_model(self.m, setter, args)
        if setter == "load_camera" and args[0] == "plumb_bob":
            self.plumb_bob_used = True
        if setter == "set_ccc_model":          # the header is silent about the filter state across a swap: a reset follows, on both sides
            self.emit("reset_white_balance_temporal_consistency", ())
        elif setter != "reset_white_balance_temporal_consistency":
            self.prev = (setter, before, head) if before is not None and before != args else self.prev

    def applicable(self, setter):
        return setter != "set_ccc_model" or self.m["wb_method"] == "ccc"      # where the reset that follows a swap arms

    def draw_args(self, setter, same=False):
        m = self.m
        if same and setter != "set_tunable":
            cur = current_args(m, setter)
            if cur is not None:
                return cur
        if setter in SCALAR:
            cur, values = m[SCALAR[setter][0]], SCALAR[setter][1]
            v = self.pick(values, setter)
            return (v if v != cur else self.pick(values, setter),)
        if setter in SPREAD:
            cur, values = current_args(m, setter), SPREAD[setter][1]
            return self.pick([v for v in values if tuple(v) != cur], setter)
        if setter in HEAD:
            field, values, spread = HEAD[setter]
            cur = getattr(m["heads"][m["selected"]], field)
            if setter == "set_output_format" and self.rng.random() < 0.5:        # the planar formats carry a table
                values = R.TABLE_FORMATS
            v = self.pick([v for v in values if v != cur], setter + str(len(values)))
            return tuple(v) if spread else (v,)
        if setter == "set_output_heads":
            return (self.pick([v for v in range(1, MAX_HEADS + 1) if v != m["n_heads"]], setter),)
        if setter == "select_output_head":
            others = [k for k in range(m["n_heads"]) if k != m["selected"]]
            return (self.pick(others, setter),) if others else (m["selected"],)
        if setter == "load_camera":
            if not self.plumb_bob_used and self.rng.random() < 0.15:
                return ("plumb_bob",) + self.pick(CAM_GEOMETRIES[:2])
            return ("equidistant",) + self.pick([g for g in CAM_GEOMETRIES if m["cam"] is None or g != m["cam"][1:]], setter)
        if setter == "set_ccc_model":
            return ("default" if m["ccc_model"] == "synthetic" else "synthetic",)
        if setter == "set_tunable":
            self.tunable_serial += 1
            name = list(TUNABLES)[(self.seed + self.tunable_serial) % len(TUNABLES)]
            cur = dict(m["tunables"])[name]
            return (name, cur if same else self.pick([v for v in TUNABLES[name] if v != cur], name))
        if setter == "set_stream":
            return (self.pick([v for v in (0, 1, 2) if v != m["stream"]], setter),)
        return ()

    def mutate(self):
        r = self.rng.random()
        if r < 0.18 and not self.must_mutate and self.prev is not None and (self.prev[0] not in HEAD or self.prev[2] == self.m["selected"]):
            setter, args, _ = self.prev          # A -> B -> A: most keys are only wrong on the way back
            if setter == "select_output_head" and args[0] >= self.m["n_heads"]:
                return
            if self.applicable(setter) and (setter != "load_camera" or args is not None):
                self.prev = None
                self.emit(setter, args, "revert")
                self.prev = None
                return
        if self.must_mutate:
            setter = self.must_mutate.pop()
            if isinstance(setter, tuple):
                self.emit(*setter)
                return
            if setter == "set_ccc_model":
                self.require("set_white_balance_method", ("ccc",))
        else:
            setter = self.pick(self.theme.boost) if self.rng.random() < 0.5 else self.pick(MUTATION_KINDS)
        if not self.applicable(setter):
            return
        same = self.rng.random() < 0.15 and setter not in ("reset_white_balance_temporal_consistency", "set_ccc_model") and \
            (setter != "load_camera" or self.m["cam"] is not None)
        self.emit(setter, self.draw_args(setter, same), "same" if same else "")
        if self.rng.random() < 0.3:              # a second mutation of the same cache with no frame in between
            rows = rows_of_mutation(setter)
            if rows:
                row = CACHES[self.pick(rows)]
                others = [s for s in row.stale + row.keep if not s.startswith("call:") and self.applicable(s)]
                if others:
                    second = self.pick(others, "double")
                    self.emit(second, self.draw_args(second), "double")

    # -- calls
    def ensure_input(self, over):
        """The mutations without which the library refuses the input a walk must draw."""
        kind, size = over.get("kind"), over.get("size")
        if kind in BAYER16 and not self.m["debayer_16bit"]:
            self.emit("set_debayer_16bit", (True,))
        if kind in BAYER16 and self.m["range16"] == (0, 0) and (self.m["wb"] or self.m["cc"] or self.m["gamma"] or self.m["vig"] or self.m["ce"] or remapped(self.m)):
            self.emit("set_debayer_16bit_range", (64, 1023))
        if kind == "mono8" and self.m["vig"]:
            self.emit("set_vignetting_correction", (False,))
        if size in CAM_GEOMETRIES:
            self.require("load_camera", ("equidistant",) + size)
            self.require("set_undistortion", (True,))
        elif size is not None and remapped(self.m):
            self.emit("set_undistortion", (False,))

    def draw_call(self, kind=None, size=None):
        m, rng = self.m, self.rng
        kind = kind or self.pick(self.theme.kinds if rng.random() < 0.7 else INPUT_KINDS)
        if size is None:
            if remapped(m):
                size = m["cam"][1:]
            else:
                size = self.pick(self.theme.geometries if rng.random() < 0.7 else GEOMETRIES + CAM_GEOMETRIES[:1] + CCC_GEOMETRIES[:1])
        layout = input_form(kind)[2]
        if layout:
            size = (PKR.allowed_width(size[0], layout), size[1])
        n = self.pick(BATCHES)
        # What the CPU expectation costs: a drawn call of 720 x 540 frames holds at most 2 of them, one above 150 x 100 at most 9.  The
        # batch sizes that cross ccc_argmax_in_finalize and the LDS-histogram threshold (13, 17) therefore reach the ccc estimator at
        # 384 x 240 only, in the directed call:larger and call:cccN runs; 720 x 540 (the exact 2 x 2 shrink) never sees a batch beyond 2.
        if size[0] * size[1] > 400 * 300:
            n = min(n, 2)
        elif size[0] * size[1] > 150 * 100:
            n = min(n, 9)
        entry = self.pick(self.theme.entries if rng.random() < 0.6 else ENTRIES)
        heads = []
        if entry in ("apply_device_heads", "apply_heads"):
            heads = [k for k in range(m["n_heads"]) if rng.random() < 0.7] or [int(rng.integers(m["n_heads"]))]
        after = []
        if entry not in ("apply_heads", "submit_collect") and not is_bgr16(m, kind):
            if wb_mode(m, kind) in ("grey_world", "simple", "ccc") and rng.random() < 0.6:
                after.append("wb_info")
        if m["rect_mask"] != "off" and not is_bgr16(m, kind) and rng.random() < 0.8:
            after += ["rect_mask"] + (["output_mask"] if not heads or m["selected"] in heads else [])
        self.call_serial += 1
        return dict(kind=kind, size=tuple(size), n=n, entry=entry, seed=1000 * self.seed + self.call_serial, heads=heads,
                    layout=self.pick(("pitch16", "frame_gap") if kind in BAYER16 else H.LAYOUTS[1:]), dest=[self.pick(("tight", "elem", "p16")) for _ in range(m["n_heads"])],
                    taps=bool(entry in ("apply_device", "apply_device_strided", "apply_device_heads") and kind != "mono8" and not is_bgr16(m, kind) and rng.random() < 0.5),
                    after=after, refusal=None)

    def repair(self, call, refusal):
        """Single mutations that take the refusing head back to what every frame accepts."""
        k = refusal["head"]
        if k is None:
            return
        if k != self.m["selected"]:
            self.emit("select_output_head", (k,))
        for setter, args in (("set_output_roi", (0, 0, 0, 0)), ("set_output_interpolation", ("linear",)), ("set_output_format", ("native",)), ("set_output_size", (0, 0))):
            if current_args(self.m, setter) != args:
                self.emit(setter, args)
            if probe_refusal(self.probe, self.m, dict(call, heads=[k], entry="apply_device_heads")) is None:
                return

    def force_refusal(self, cls=None):
        """The mutations that make the next call one the library refuses, and that call; False where the model does not allow the class."""
        m = self.m
        forced = cls
        stages_off = not (m["wb"] or m["cc"] or m["gamma"] or m["vig"] or m["ce"] or remapped(m))
        if self.theme.name == "raw16" and stages_off:          # a bgr16 result exists only while every 8-bit stage is off
            cls = REFUSAL_CLASSES[4 + (self.seed // len(THEMES) + self.refusals) % 3]
        else:
            cls = REFUSAL_CLASSES[(self.seed + self.refusals) % 4]
        cls = forced or cls
        kind, size, entry, heads, taps = self.pick(BAYER8), None, self.pick(("apply_device", "process", "apply_device_heads")), None, None
        if cls == "area_upscale":
            self.emit("set_output_interpolation", ("area",))
            self.emit("set_output_size", (1500, 1100))
        elif cls == "aa_factor":
            self.emit("set_output_interpolation", (self.pick(("linear_aa", "cubic_aa")),))
            self.emit("set_output_size", (1, 1))
            size = None if remapped(m) else (136, 72)
        elif cls == "roi_outside":
            self.emit("set_output_roi", (1000, 0, 64, 32))
        elif cls == "format_on_mono":
            if m["vig"]:
                self.emit("set_vignetting_correction", (False,))
            self.emit("set_output_format", (self.pick(("rgb8",) + R.TABLE_FORMATS),))
            kind = "mono8"
        else:
            kind = self.pick(BAYER16)
            if not m["debayer_16bit"]:
                self.emit("set_debayer_16bit", (True,))
            if m["range16"] != (0, 0):
                self.emit("set_debayer_16bit_range", (0, 0))
            if cls == "bgr16_format":
                self.emit(*self.pick((("set_output_format", ("rgb8",)), ("set_output_size", (32, 24)))))
            else:
                entry = "apply_device_heads"
                if cls == "bgr16_heads":
                    if m["n_heads"] < 2:
                        self.emit("set_output_heads", (2,))
                    heads, taps = [0, 1], False
                else:
                    heads, taps = [self.m["selected"]], True
        call = self.draw_call(kind, size)
        call["entry"] = entry
        call["after"] = []
        if entry == "apply_device_heads":
            call["heads"] = heads if heads is not None else [self.m["selected"]]
            call["taps"] = bool(taps) if taps is not None else call["taps"] and not is_bgr16(self.m, kind)
        else:
            call["heads"], call["taps"] = [], False
        refusal = probe_refusal(self.probe, self.m, call)
        if refusal is None:
            return False
        call["refusal"] = {k: refusal[k] for k in ("status", "prefix", "cls")}
        self.steps.append(("call", call))
        self.calls += 1
        self.refusals += 1
        return True

    def settle(self, call):
        """Repairs head after head until the call is accepted; returns the refusal that no head setting explains (or None)."""
        refusal = None
        for _ in range(MAX_HEADS + 1):
            refusal = probe_refusal(self.probe, self.m, call)
            if refusal is None or refusal["cls"] == "other" or refusal["head"] is None:
                break
            self.repair(call, refusal)
        return refusal

    def call(self):
        share = 0.2 if self.theme.name == "raw16" else 0.055
        if self.calls >= (3 if self.theme.name == "raw16" else 6) and self.refusals < share * (self.calls + 1) and self.force_refusal():
            return
        call = refusal = None
        over = self.must_call.pop() if self.must_call else {}
        self.ensure_input(over)
        for _ in range(6):
            call = self.draw_call(over.get("kind"), over.get("size"))
            call.update({k: v for k, v in over.items() if k in ("entry", "n", "layout")})
            if "entry" in over:
                call["heads"] = [k for k in range(self.m["n_heads"]) if k != self.m["selected"] or self.m["n_heads"] == 1] if over["entry"] in ("apply_device_heads", "apply_heads") else []
                call["taps"] = call["taps"] and over["entry"] in ("apply_device", "apply_device_strided", "apply_device_heads")
                call["after"] = [a for a in call["after"] if a == "rect_mask"]
            refusal = probe_refusal(self.probe, self.m, call)
            if refusal is None:
                break
        if refusal is not None:
            refusal = self.settle(call)
        if refusal is not None:                  # the input itself is refused (a 16-bit frame without the switch, vignetting on one channel ..)
            call = self.draw_call(self.pick(BAYER8), call["size"] if input_form(call["kind"])[2] is None else None)
            refusal = self.settle(call)
        assert refusal is None, (self.seed, call, refusal)
        self.steps.append(("call", call))
        self.calls += 1

    # -- directed runs: fill -> the staling kind -> read (-> back again -> read) for the pairs of CACHES this walk is responsible for
    def require(self, setter, args):
        if setter == "set_tunable":
            if dict(self.m["tunables"])[args[0]] != args[1]:
                self.emit(setter, args)
        elif current_args(self.m, setter) != tuple(args):
            self.emit(setter, args)

    def fixed_call(self, spec):
        call = self.draw_call(spec["kind"], None if remapped(self.m) else spec["size"])
        call.update(n=spec["n"], entry=spec["entry"], heads=list(spec.get("heads", [])), taps=bool(spec.get("taps")))
        call["after"] = [a for a in spec["after"] if (wb_mode(self.m, call["kind"]) in ("grey_world", "simple", "ccc") if a == "wb_info" else self.m["rect_mask"] != "off")]
        if self.settle(call) is not None:
            return False
        self.steps.append(("call", call))
        self.calls += 1
        return True

    def showcase(self):
        """One call per walk that delivers a resized head under this walk's share of the interpolations, fit modes and formats, after
        one under its share of the estimators."""
        r = self.seed % len(DEFAULT_SEEDS)
        method = (None, "grey_world", "pca", "simple")[r % 4]
        if method is not None:
            self.require("set_white_balance", (True,))
            self.require("set_white_balance_method", (method,))
            self.fixed_call(dict(kind=BAYER8[r % 4], size=GEOMETRIES[r % 3], n=2, entry="apply_device", after=["wb_info"], taps=True))
        heads = []
        if r % 4 == 0:
            self.require("set_output_heads", (3,))
            heads = [self.m["selected"], (self.m["selected"] + 1) % 3]
        self.require("set_output_interpolation", (INTERPOLATIONS[r % 4],))
        self.require("set_output_size", (96, 64))
        self.require("set_output_fit", (FITS[r % 3],))
        self.require("set_output_format", (FORMATS[r % len(FORMATS)],))
        entry = "apply_device_heads" if heads else ("process", "apply_device", "submit_collect")[r % 3]
        self.fixed_call(dict(kind=BAYER8[r % 4], size=(136, 72), n=2, entry=entry, after=[], heads=heads))

    def prepare(self, row, kind):
        """The mutations after which a call reads `row`, and that call."""
        m, req = self.m, self.require
        spec = dict(kind=self.pick(BAYER8), size=self.pick(GEOMETRIES), n=self.pick((2, 3)), entry=self.pick(("process", "apply_device", "apply_device_strided", "submit_collect")), after=[])
        camera_rows = ("maps", "plan", "plan.items", "d_mid.cap")
        if row in camera_rows or (row.startswith("mask") and kind != "call:geometry"):
            if row == "plan.items":                     # 328 x 200 at balance 0: the footprint is smaller than the frame, the chain walks its items
                req("load_camera", ("equidistant",) + CAM_GEOMETRIES[0])
                req("set_tunable", ("chain_footprint", 1))
                req("set_undistortion_balance", (0.0,))
                req("set_undistortion_fov_scale", (1.0,))
                # the stage set of tests/test_chain_footprint_gpu.py: the chain writes the intermediate image, the remap is a kernel of its own
                for setter, args in (("set_white_balance", (True,)), ("set_white_balance_method", ("grey_world",)), ("set_color_calibration", (True,)),
                                     ("set_gamma_correction", (True,)), ("set_vignetting_correction", (True,)), ("set_debayer_method", ("bilinear",))):
                    req(setter, args)
                spec.update(entry="apply_device", n=3)
                if kind == "set_flip_angle":            # from no turn to a half turn: the plan stays, the item list must not
                    req("set_flip", (True,))
                    req("set_flip_angle", (0,))
            elif m["cam"] is None:
                req("load_camera", ("equidistant",) + self.pick(CAM_GEOMETRIES[:2]))
            req("set_undistortion", (True,))
            if row.startswith("mask"):
                req("set_undistortion_balance", (1.0,))  # a coverage that is not all 255
        elif remapped(m) and (row.startswith("ccc") or row.startswith("d_") or kind == "call:geometry"):
            req("set_undistortion", (False,))
        if row.startswith("mask"):
            if m["rect_mask"] == "off":
                req("set_rect_mask", ("coverage",))
            spec.update(kind=self.pick(("mono8",) + BAYER8), entry="process", after=["rect_mask", "output_mask"])
            if kind != "set_output_roi":                 # all of the coverage: a corner of it is constant
                req("set_output_roi", (0, 0, 0, 0))
            if kind in ("set_output_interpolation", "set_output_fit", "set_output_roi"):
                req("set_output_interpolation", ("linear",))
                req("set_output_size", (96, 64))
            if m["vig"] and spec["kind"] == "mono8":
                req("set_vignetting_correction", (False,))
        if row == "tables":
            req("set_gamma_correction", (True,))
        elif row == "vignette":
            req("set_vignetting_correction", (True,))
            if kind == "set_fp_contraction":           # the stages whose fused forms round differently, at their non-neutral gains
                for setter, args in (("set_color_calibration", (True,)), ("set_color_enhancer", (True,)), ("set_color_enhancer_hue_gain", (1.3,)),
                                     ("set_color_enhancer_saturation_gain", (0.7,)), ("set_color_enhancer_value_gain", (1.1,))):
                    req(setter, args)
                spec.update(size=(136, 72), n=3)
        elif row.startswith("ccc") or row == "d_hist.clean_bytes":
            req("set_white_balance", (True,))
            req("set_white_balance_method", ("ccc",))
            spec.update(size=CCC_GEOMETRIES[0], entry="apply_device", after=["wb_info"], n=1 if row == "d_hist.clean_bytes" else 3)
            if row == "ccc.state":
                req("set_white_balance_temporal_consistency", (kind != "set_white_balance_temporal_consistency",))
                if m["kalman"][0] == 0.0:
                    req("set_ccc_kalman_model", (1.0, 10.0))
        elif row == "d_stats.clean_bytes":
            req("set_white_balance", (True,))
            req("set_white_balance_method", (self.pick(("grey_world", "pca")),))
            spec.update(after=["wb_info"], entry="apply_device")
        elif row == "d_mht.cap":
            req("set_debayer_method", ("mht",))
        elif row in ("out_table[k]", "d_fmt.cap", "d_rsz.cap"):
            if self.m["heads"][self.m["selected"]].format not in R.TABLE_FORMATS:
                req("set_output_format", (self.pick(R.TABLE_FORMATS),))
            if row == "d_rsz.cap":
                req("set_output_interpolation", ("linear",))
                req("set_output_size", (96, 64))
        if row == "rsz_tables[k]":
            if kind != "set_output_interpolation":
                req("set_output_interpolation", ("linear",))
            req("set_output_size", (96, 64))           # no geometry of the list has its aspect: the fit modes differ
            spec.update(size=(136, 72))                # a downscale on both axes: every interpolation accepts it
        return spec

    def idle(self, row, variant):
        """Mutations of `row`'s cache that leave the settings as they are: the same value again, or there and back with no frame between."""
        # of the row's `keep` list where that has one: the run's own staling kind then meets a cache nothing else has rebuilt
        setters = [k for k in CACHES[row].keep if not k.startswith("call:") and k not in SPECIAL] or \
                  [k for k in CACHES[row].stale if not k.startswith("call:") and k not in SPECIAL]
        if not setters:
            return
        setter = self.pick(setters, "idle" + row)
        now = current_args(self.m, setter)
        if variant == 1:
            self.emit(setter, now, "same")
        else:
            self.emit(setter, self.draw_args(setter))
            self.emit(setter, now, "double revert")

    def directed(self, row, kind, variant):
        """fill -> the staling kind -> read; variant 0: then back again and one more read (most keys are only wrong on the way back),
        1: a same-value set on the way, 2: two mutations of the cache with no frame between them."""
        spec = self.prepare(row, kind)
        if not self.fixed_call(spec):
            return
        first = kind == CACHES[row].stale[0]          # the row's first pair also carries its same-value set and its double mutation
        if kind.startswith("call:"):
            if first:
                self.idle(row, 1)
                self.idle(row, 2)
            if kind == "call:geometry":
                spec = dict(spec, size=self.pick([g for g in GEOMETRIES + CCC_GEOMETRIES[:1] if g != spec["size"]]))
            elif kind == "call:larger":                      # more bytes than any call of the walk so far
                largest = max([call_bytes(st[1]) for st in self.steps if st[0] == "call" and st[1]["refusal"] is None] or [0])
                for size, n in ((spec["size"], 17), ((136, 72), 17), ((384, 240), 9), ((384, 240), 17), ((720, 540), 9)):
                    if remapped(self.m):
                        size = self.m["cam"][1:]
                    if size[0] * size[1] * (min(n, RING_DEPTH) if spec["entry"] in HOST_ENTRIES else n) > largest:
                        break
                spec = dict(spec, size=size, n=n, entry="apply_device" if spec["entry"] in HOST_ENTRIES else spec["entry"])
            elif kind == "call:cccN":
                self.fixed_call(dict(spec, n=self.pick((9, 13))))
            else:
                assert kind == "call:simple", kind
                back = self.m["wb_method"]
                self.emit("set_white_balance_method", ("simple",))
                self.fixed_call(dict(spec, after=[]))
                self.emit("set_white_balance_method", (back,))
            self.fixed_call(spec)
            return
        back = current_args(self.m, kind)
        if kind == "load_camera" and not self.plumb_bob_used:      # another camera of the SAME size: without it the frame is still one the old maps take
            self.emit(kind, ("plumb_bob",) + self.m["cam"][1:])
        elif kind == "set_flip_angle" and row == "plan.items":
            self.emit(kind, (180,))
        elif kind == "set_output_format" and row == "out_table[k]":  # from one planar format to another: the table is read before and after
            self.emit(kind, (self.pick([f for f in R.TABLE_FORMATS if f != back[0]]),))
        else:
            self.emit(kind, self.draw_args(kind))
        if first:
            self.idle(row, 1)
            self.idle(row, 2)
        self.fixed_call(spec)
        if variant != 1 and back is not None and kind not in ("set_ccc_model", "reset_white_balance_temporal_consistency"):
            self.emit(kind, back, "revert")
            self.fixed_call(spec)
        if (row, kind) == ("rsz_tables[k]", "set_output_interpolation"):
            # linear, then area, at one (R, C, H, W) with the window twice the picture: both are the 2 x 2 mean of one table set (key kind 0)
            self.require("set_output_roi", (0, 0, 0, 0))
            self.require("set_output_interpolation", ("linear",))
            f_size = self.m["cam"][1:] if remapped(self.m) else spec["size"]           # F: the maps' size, else the frame's (no quarter turn below)
            if not remapped(self.m) and effective_flip(self.m) in (90, 270):
                self.emit("set_flip", (False,))
            self.require("set_output_size", (f_size[0] // 2, f_size[1] // 2))
            self.fixed_call(spec)
            self.emit("set_output_interpolation", ("area",))
            self.fixed_call(spec)
        self.prev = None

    def run(self):
        for setter, args in self.theme.start:
            self.emit(setter, args)
        self.prev = None
        if self.theme.name == "raw16":                       # a bgr16 result exists only while every 8-bit stage is off: its refusals come first
            for j in range(2):
                self.must_call.append(dict(kind=BAYER16[(self.seed + j) % 4]))
                self.call()
                self.force_refusal(REFUSAL_CLASSES[4 + (self.seed // len(THEMES) + j) % 3])
        self.showcase()
        agenda = [pair for i, pair in enumerate(PAIRS) if i % len(DEFAULT_SEEDS) == self.seed % len(DEFAULT_SEEDS)]
        done = 0
        while len(self.steps) < self.n_steps + 1 or done < len(agenda) or self.must_mutate or self.must_call:
            owed = self.must_mutate or self.must_call
            if done < len(agenda) and len(self.steps) >= min(self.n_steps, 8 + done * (self.n_steps - 8) // len(agenda)):
                self.directed(*agenda[done], variant=(self.seed + done) % 3)
                done += 1
            elif owed and (len(self.steps) % 3 == 0 or len(self.steps) > self.n_steps):      # what the walk owes, between what the dice draw
                if self.must_mutate and (not self.must_call or len(self.steps) % 2):
                    self.mutate()
                else:
                    self.call()
            elif self.rng.random() < 0.55:
                self.mutate()
            else:
                self.call()
        return self.steps


@functools.lru_cache(maxsize=None)
def _walk(seed, n_steps):
    return tuple(Walker(seed, n_steps).run())


def walk(seed, n_steps=DEFAULT_STEPS):
    """The steps of walk `seed`: at least n_steps + 1 of them, the first ("init",)."""
    return list(_walk(seed, n_steps))


def walk_from(steps):
    """[(step, model after it)] of a printed list of steps."""
    return [(step, m) for step, m, _, _ in annotate(steps)]


def format_steps(steps):
    return "[\n" + "".join("  %r,\n" % (s,) for s in steps) + "]"


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _frame(kind, w, h, seed):
    tint = (0.60 + 0.05 * (seed % 8), 1.0, 0.55)
    cn, _, layout, wide = input_form(kind)
    if kind in BAYER8:
        f = synth.gen_frame(w, h, kind, seed=seed, kind="scene", tint=tint)
    elif kind in ("bgr8", "rgb8"):
        f = synth.gen_scene_bgr(w, h, seed, tint)
        f = np.ascontiguousarray(f[..., ::-1]) if kind == "rgb8" else f
    elif kind == "mono8":
        f = synth.gen_scene_bgr(w, h, seed, tint)[..., 1].copy()
    elif wide:
        f = G.gen_frame16(w, h, kind[6:10], seed, 64, 1023, tint=tint)
    else:
        top = (1 << PKR.BITS[layout]) - 1
        f = PKR.pack(np.minimum(G.gen_frame16(w, h, kind[6:10], seed, 64, top, tint=tint), top).astype(np.uint16), layout)
    f = np.ascontiguousarray(f)
    f.setflags(write=False)
    return f


def frames(call):
    """The host frames of a call: uint8 [rows, cols(, 3)], uint16 [rows, cols], or packed rows uint8 [rows, row bytes]."""
    w, h = call["size"]
    return [_frame(call["kind"], w, h, call["seed"] + i) for i in range(frame_count(call))]


# ---- the expectation -------------------------------------------------------------------------------------------------------------------
def delivered_encoding(f_enc, channels, head):
    if head.format == "native":
        return f_enc
    return "mono8" if channels == 1 else head.format


def deliver(F, head, mask=False):
    """What a head delivers for the pipeline's image F: window and picture by fit_reference.geometry, the picture by the filter's
    reference, the rest pad, the format on top.  mask: one channel, pad 0, format native (PARITY.md "Rect mask")."""
    F = np.asarray(F)
    if F.dtype == np.uint16:
        return F                                       # bgr16: only the identity is accepted
    rows, cols = F.shape[:2]
    channels = 1 if F.ndim == 2 else 3
    (x, y, w, h), (left, top, wi, hi), (W, Hh) = FR.geometry(cols, rows, head.roi, head.size, head.fit)
    window = np.ascontiguousarray(F[y:y + h, x:x + w])
    if (h, w) == (hi, wi):
        pic = window
    elif head.interp in AA.FILTERS:
        pic = AA.resize(window, hi, wi, head.interp)
    else:
        pic = FR.picture(window, hi, wi, head.interp)
    canvas = np.empty((Hh, W) + F.shape[2:], np.uint8)
    canvas[...] = np.array(FR.pad_bytes((0, 0, 0) if mask else head.pad, channels), np.uint8)
    canvas[top:top + hi, left:left + wi] = pic
    if mask or head.format == "native" or channels == 1:
        return canvas
    return R.convert(canvas[None], head.format, *head.norm)[0]


Expected = collections.namedtuple("Expected", ["F", "f_enc", "heads", "encodings", "taps", "estimates", "rect_mask", "output_mask", "mid"])


class Evaluator:
    """The CPU expectation of a walk.  Holds what the settings do not: the oracle's ccc objects -- per model the one the oracle's
    pipeline advances and a twin that is fed the same images and yields the track and the gains."""

    def __init__(self, O):
        self.O = O
        self.occ = {name: [O.CCC(*D.model_arrays(name)) for _ in range(2)] for name in D.CCC_MODELS}
        self._map_cache = {}
        self.set_kalman(*initial_model()["kalman"])

    def set_kalman(self, h, r):
        for pair in self.occ.values():
            for o in pair:
                o.set_kalman_model(h, r)

    def mutation(self, m_before, setter, args):
        if setter == "set_ccc_kalman_model":
            self.set_kalman(*args)
        elif setter == "reset_white_balance_temporal_consistency" and m_before["wb_method"] == "ccc":     # rip_api.cpp: armed only then
            for pair in self.occ.values():
                for o in pair:
                    o.reset()

    def _maps(self, m):
        key = (m["cam"], m["balance"], m["fov_scale"])
        if key not in self._map_cache:
            cam = camera(m["cam"])
            size = (cam["width"], cam["height"])
            if m["cam"][0] == "equidistant":
                mx, my = H.oracle_maps(self.O, dict(cam=cam, balance=m["balance"], fov_scale=m["fov_scale"]))
            else:
                newK = PR.new_camera_matrix(cam["K"], "plumb_bob", cam["D"], size, m["balance"], None, m["fov_scale"])
                mx, my = PR.maps(cam["K"], "plumb_bob", cam["D"], cam["R"], newK, size)
            if len(self._map_cache) > 8:
                self._map_cache.clear()
            self._map_cache[key] = (np.ascontiguousarray(mx, np.float32), np.ascontiguousarray(my, np.float32))
        return self._map_cache[key]

    def _pinhole_run(self, m, c, image, encoding, ccc):
        """helpers.oracle_run with the undistortion reading the plumb_bob maps (as tests/test_pinhole_gpu.py does)."""
        keep = []
        prm = H.oracle_params(self.O, c, keep)
        if m["undistort"]:
            mx, my = self._maps(m)
            prm.und_enabled = 1
            prm.map_x, prm.map_y = mx.ctypes.data, my.ctypes.data
            prm.map_rows, prm.map_cols = mx.shape
        return self.O.pipeline(prm, np.ascontiguousarray(image), encoding, ccc=ccc, taps=True)

    def _frame(self, m, kind, frame, width, ccc):
        """(F, encoding, debayered tap, colour tap) of one frame; the taps None for a bgr16 result."""
        O, c = self.O, cfg_of(m)
        _, _, layout, wide = input_form(kind)
        name, method = kind[6:10], m["debayer_method"]
        if layout:
            frame = PKR.unpack(frame, width, layout)
        if is_bgr16(m, kind):
            return MF.flip(demosaic16(O, frame, name, method), effective_flip(m)), "bgr16", None, None
        rng16 = m["range16"] if m["range16"] != (0, 0) else (PKR.natural_range(layout) if layout else None)
        pinhole = m["cam"] is not None and m["cam"][0] == "plumb_bob"
        with O.fp_contraction(m["fp_contract"]):
            if pinhole:
                if wide or layout:
                    image, enc = narrow16(demosaic16(O, frame, name, method), *rng16), "bgr8"
                elif kind in BAYER8 and method == "mht":
                    image, enc = MF.mht_reference(frame, kind), "bgr8"
                else:
                    image, enc = frame, kind
                return self._pinhole_run(m, c, image, enc, ccc)
            if wide or layout:
                return expected_raw16(O, c, frame, name, method, rng16[0], rng16[1], ccc=ccc, taps=True)
            if kind in BAYER8 and method == "mht":
                return H.expected_mht(O, c, frame, kind, ccc=ccc, taps=True)
            return H.oracle_run(O, c, frame, kind, ccc=ccc, taps=True)

    def expected(self, m, call, frame_list=None):
        """What the accepted call must deliver under model m.  Advances the ccc objects when the call runs the ccc estimator."""
        frame_list = frames(call) if frame_list is None else frame_list
        kind = call["kind"]
        w, h = call["size"]
        assert not remapped(m) or (w, h) == m["cam"][1:], "the oracle's buffers take undistorted frames of the calibration's size only"
        mode = wb_mode(m, kind)
        swap = effective_flip(m) in (90, 270)
        mid = (w, h) if swap else (h, w)               # rows, cols after the flip
        Fs, taps, estimates, f_enc = [], ([], []), [], None
        for frame in frame_list:
            active = self.occ[m["ccc_model"]] if mode == "ccc" else None
            F, f_enc, t0, t1 = self._frame(m, kind, frame, w, active[0] if active else None)
            Fs.append(F)
            est = None
            if t0 is not None and kind != "mono8":
                t0, t1 = (np.asarray(t)[:mid[0] * mid[1] * 3].reshape(mid[0], mid[1], 3) for t in (t0, t1))
                taps[0].append(t0)
                taps[1].append(t1)
                if mode == "ccc":
                    params = dict(wb_bright=m["wb_bright"], wb_dark=m["wb_dark"])
                    for name, pair in self.occ.items():
                        for o in pair[1:] if pair is active else pair:
                            o.set_temporal_consistency(m["wb_temporal"])
                            e = D.expected(self.O, "ccc", params, "bgr8", t0, occ=o)
                            if pair is active:
                                est = e.estimate
                elif mode in ("grey_world", "simple"):
                    est = D.expected(self.O, mode, dict(wb_bright=m["wb_bright"], wb_percentile=m["wb_percentile"]), "bgr8", t0).estimate
            estimates.append(est)
        channels = 1 if Fs[0].ndim == 2 else 3
        heads, encodings = {}, {}
        for k in delivered_heads(m, call):
            heads[k] = np.stack([deliver(F, m["heads"][k]) for F in Fs])
            encodings[k] = delivered_encoding(f_enc, channels, m["heads"][k])
        rect_mask = output_mask = None
        if m["rect_mask"] != "off" and Fs[0].dtype == np.uint8:
            base = None
            if remapped(m):
                base = MC.expected(self.O, *self._maps(m), (mid[1], mid[0]))
            rect_mask = np.empty((0, 0), np.uint8) if base is None else base
            if "output_mask" in call["after"]:        # of the selected head, which a heads call need not have delivered
                output_mask = deliver(base if base is not None else np.full(Fs[0].shape[:2], 255, np.uint8), m["heads"][m["selected"]], mask=True)
            if m["rect_mask"] == "valid":
                rect_mask = MC.valid_of(rect_mask) if base is not None else rect_mask
                output_mask = MC.valid_of(output_mask) if output_mask is not None else None
        return Expected(Fs, f_enc, heads, encodings, (np.stack(taps[0]), np.stack(taps[1])) if taps[0] else None, estimates, rect_mask, output_mask, mid)

    def replay(self, steps):
        """Yields (index, step, model after the step, Expected or None) for every step; None for mutations and refusals."""
        m = None
        for i, step in enumerate(steps):
            e = None
            if step[0] == "init":
                m = initial_model()
            elif step[0] == "mut":
                self.mutation(m, step[1], step[2])
                m = update_model(m, step[1], step[2])
            elif step[1]["refusal"] is None:
                e = self.expected(m, step[1])
            yield i, step, m, e


def expected(model, call, frames, evaluator=None):
    """The expectation of one call under `model`.  evaluator: the Evaluator that carries the ccc filter state of the walk so far; without
    one the call is the first the estimator sees."""
    if evaluator is None:
        import oracle
        evaluator = Evaluator(oracle)
    return evaluator.expected(model, call, frames)


def digest(e, masks_only=False):
    """A hashable summary of everything an Expected asserts about delivered bytes (masks_only: about the masks)."""
    import hashlib
    h = hashlib.sha1()
    for k in sorted(e.heads) if not masks_only else ():
        h.update(repr((k, e.heads[k].shape, str(e.heads[k].dtype), e.encodings[k])).encode())
        h.update(np.ascontiguousarray(e.heads[k]).tobytes())
    for m in (e.rect_mask, e.output_mask):
        if m is not None:
            h.update(repr(m.shape).encode() + np.ascontiguousarray(m).tobytes())
    return h.hexdigest()


def expected_without(O, steps, k, a):
    """The expectation of call step `a` had step `k` never happened -- what a handle delivers whose caches did not notice step k.
    Calls in front of `a` are evaluated only where they move the ccc filter state.  None where the library would refuse the call
    without step k (a probe handle decides, as in the walk)."""
    if k is not None:
        probe, m = new_probe(), initial_model()
        for i, step in enumerate(steps[:a]):
            if i != k and step[0] == "mut":
                apply_mutation(probe, step[1], step[2])
                m = update_model(m, step[1], step[2])
        if probe_refusal(probe, m, steps[a][1]) is not None:
            return None
        if remapped(m) and steps[a][1]["size"] != m["cam"][1:]:      # the walks undistort frames of the calibration's size only
            return None
    ev, m, e = Evaluator(O), None, None
    for i, step in enumerate(steps[:a + 1]):
        if i == k:
            continue
        if step[0] == "init":
            m = initial_model()
        elif step[0] == "mut":
            ev.mutation(m, step[1], step[2])
            m = update_model(m, step[1], step[2])
        elif step[1]["refusal"] is None and (i == a or wb_mode(m, step[1]["kind"]) == "ccc"):
            if remapped(m) and step[1]["size"] != m["cam"][1:]:
                return None
            e = ev.expected(m, step[1])
    return e
