"""Degenerate frames for the white-balance estimators: the cases of tests/test_wb_degenerate_cases.py (CPU) and
tests/test_wb_degenerate_gpu.py (PARITY.md "Degenerate frames").

synth.gen_frame gives scenes around a mean of 110 and iid bytes: no statistic is ever zero, no determinant small, no histogram
empty, no accumulator near its range.  The content kinds here are the frames where those things happen -- lens cap on, night, a
blown-out sky, a single-colour wall, a dead channel -- as BGR images that are a pure function of (kind, size, input form).

Importable without a GPU and without torch; nothing here looks at the library.  The functions that evaluate a case take the
oracle module as a parameter."""
import collections
import os

import numpy as np

from raw_image_pipeline_amd import synth

REF_WB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference", "white_balance")

KINDS = ("black", "white", "flat_grey", "flat_colour", "zero_channel", "full_channel", "const_channel", "flat_plus_one_pixel",
         "lens_cap", "blown", "primaries", "blown_with_patch")
FORMS = ("bgr8", "rgb8", "bayer_rggb8", "bayer_grbg8", "bayer_gbrg8", "bayer_bggr8")
FLAT_COLOUR = (200, 93, 17)
ONE_PIXEL = (129, 128, 127)
PATCH = 32
SEED = 77000

# (w, h) -> what launch_stats takes there (rip_stats.hip): the Bayer fast path needs cols % 4 == 0 and rows % 2 == 0, the
# four-pixels-per-lane colour path cols % 4 == 0; 51 x 33 leaves every form to the generic kernel
STAT_SIZES = ((64, 48), (132, 36), (51, 33))
# ccc shrinks every frame to 360 x 270: bilinear from 384 x 240, the exact 2 x 2 mean from 720 x 540
CCC_SIZES = ((384, 240), (720, 540))

GREY_WORLD_THRESHOLDS = (0.0, 0.5, 1.0, 1.5)     # thresh255 = 0, 128 (127.5 rounds to even), 255, 382 (clamped by the packed keep test)
SIMPLE_PERCENTILES = (0.0, 1.0, 10.0, 50.0)
CCC_THRESHOLDS = ((0.8, 0.2), (1.0, 0.0), (0.2, 0.8))   # the last pair masks every pixel: an empty histogram
CCC_MODELS = ("synthetic", "default")

# Which observable proves the estimate of a case: "image", "info" (rip_get_white_balance_info: grey-world q8, SimpleWB's alpha,
# ccc gains and (u, v); rip_get_ccc_track: the raw and filtered arg-max), "both", or "none".  pca has no getter, so its image is
# its only witness.  The image proves an estimate where a perturbed estimate changes the oracle's image
# (tests/test_wb_degenerate_cases.py: for every class of perturbation the method has -- a channel sum off by 2^32, a Q8 gain off by
# one, a (u, v) bin off by one, SimpleWB's low cut one level up -- at least one perturbed estimate must).  On the content below it
# does not in at least one form, size or setting, so those cases are proven by the getter, which the GPU test compares bit for bit
# in every case that has one:
#   black                a zero stays zero under every gain; SimpleWB maps it to 128 whatever alpha is (0 * alpha + 127.5)
#   lens_cap             values 0 and 1: (1 * q8) >> 8 is 0 for every q8 below 256, and a ccc gain below 1.5 leaves 1 at 1
#   white, blown         saturated: a ccc gain is at least 1, so 254 and 255 go to 255 under every (u, v)
#   dead channels        grey-world with a low threshold skips every pixel (all sums zero, all gains zero)
#   flat frames          SimpleWB maps a one-level channel to 128 whatever the cut
# pca on a black frame has NaN coefficients and a zero image whatever the sums are: it runs for its defined result only.
IMAGE_BLIND = {
    "grey_world": ("black", "const_channel", "flat_colour", "full_channel", "primaries", "zero_channel"),
    "simple": ("black", "blown", "blown_with_patch", "flat_colour", "flat_grey", "flat_plus_one_pixel", "white"),
    "ccc": ("black", "blown", "lens_cap", "primaries", "white"),
    "pca": ("black", "primaries"),
}

Case = collections.namedtuple("Case", ["method", "params", "model", "kind", "form", "size", "witness"])


def kind_seed(kind):
    return SEED + KINDS.index(kind)


def one_pixel_position(form, w, h):
    """Where flat_plus_one_pixel puts its pixel: near the centre, on the R site of a Bayer form (a G site would sample 128 and
    leave the mosaic exactly flat)."""
    y, x = (h // 2) & ~1, (w // 2) & ~1
    if form.startswith("bayer_"):
        cell = synth.PATTERNS[form]
        ry, rx = [(dy, dx) for dy in range(2) for dx in range(2) if cell[dy][dx] == 2][0]
        y, x = y + ry, x + rx
    return y, x


def content(kind, w, h, form="bgr8"):
    """The BGR image of a kind (uint8, h x w x 3)."""
    rng = np.random.default_rng(kind_seed(kind))
    img = np.empty((h, w, 3), np.uint8)
    if kind == "black":
        img[...] = 0
    elif kind == "white":
        img[...] = 255
    elif kind == "flat_grey":
        img[...] = 93
    elif kind == "flat_colour":
        img[...] = FLAT_COLOUR
    elif kind in ("zero_channel", "full_channel", "const_channel"):
        img[...] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if kind == "zero_channel":
            img[..., 0] = 0
        elif kind == "full_channel":
            img[..., 2] = 255
        else:
            img[..., 0] = 77
    elif kind == "flat_plus_one_pixel":
        img[...] = 128
        y, x = one_pixel_position(form, w, h)
        img[y, x] = ONE_PIXEL
    elif kind == "lens_cap":
        img[...] = rng.integers(0, 2, (h, w, 3), dtype=np.uint8)
    elif kind in ("blown", "blown_with_patch"):
        img[...] = rng.integers(254, 256, (h, w, 3), dtype=np.uint8)
        if kind == "blown_with_patch":
            y0, x0 = ((h - PATCH) // 2) & ~1, ((w - PATCH) // 2) & ~3
            img[y0:y0 + PATCH, x0:x0 + PATCH] = rng.integers(0, 256, (PATCH, PATCH, 3), dtype=np.uint8)
    elif kind == "primaries":
        img[...] = 0
        img[:, :w // 2, 0] = 255
        img[:, w // 2:, 2] = 255
    else:
        raise ValueError(kind)
    return img


def frame(kind, form, w, h):
    """What the library is handed: the BGR image, its RGB twin, or its mosaic."""
    bgr = content(kind, w, h, form)
    if form == "bgr8":
        f = bgr
    elif form == "rgb8":
        f = np.ascontiguousarray(bgr[..., ::-1])
    else:
        f = synth.mosaic(bgr, form)
    f.setflags(write=False)
    return f


def method_settings():
    """[(method, params, model)]: every estimator setting of the cases."""
    out = [("grey_world", dict(wb_bright=t), None) for t in GREY_WORLD_THRESHOLDS]
    out.append(("pca", {}, None))
    out += [("simple", dict(wb_percentile=p), None) for p in SIMPLE_PERCENTILES]
    out += [("ccc", dict(wb_bright=b, wb_dark=d), m) for m in CCC_MODELS for b, d in CCC_THRESHOLDS]
    return out


def witness_of(method, kind):
    if method == "pca":
        return "none" if kind in IMAGE_BLIND[method] else "image"
    return "info" if kind in IMAGE_BLIND[method] else "both"


def build_cases():
    cases = []
    for method, params, model in method_settings():
        for size in (CCC_SIZES if method == "ccc" else STAT_SIZES):
            for form in FORMS:
                for kind in KINDS:
                    cases.append(Case(method, params, model, kind, form, size, witness_of(method, kind)))
    return cases


CASES = build_cases()


def setting_id(method, params, model):
    return "-".join([method] + ["%g" % params[k] for k in sorted(params)] + ([model] if model else []))


def case_id(case):
    return "%s %s %s %dx%d" % (setting_id(case.method, case.params, case.model), case.kind, case.form, case.size[0], case.size[1])


def groups():
    """The cases grouped by (setting, form, size): one test each, its twelve kinds run on one handle."""
    g = collections.OrderedDict()
    for c in CASES:
        g.setdefault((setting_id(c.method, c.params, c.model), c.form, c.size), []).append(c)
    return g


def group_id(key):
    return "%s %s %dx%d" % (key[0], key[1], key[2][0], key[2][1])


def expected_stats_kernel(form, size):
    """The statistics kernel launch_stats takes for a tightly packed frame (bayer_fast_geometry / color_fast_geometry)."""
    w, h = size
    if form.startswith("bayer_") and w % 4 == 0 and h % 2 == 0:
        return "stats_fast_kernel<?>"
    if not form.startswith("bayer_") and w % 4 == 0:
        return "stats_color_kernel"
    return "stats_generic_kernel"


# ---- the ccc models ------------------------------------------------------------------------------------------------------
def default_model_path():
    return os.path.join(REF_WB, "default.bin")


def load_default_model():
    """(filter, bias) of the reference's model file: int w, int h, float filter[w * h], float bias[w * h]."""
    raw = np.fromfile(default_model_path(), dtype=np.uint8)
    w, h = (int(v) for v in np.frombuffer(raw[:8].tobytes(), dtype=np.int32))
    assert (w, h) == (256, 256) and raw.size == 8 + 2 * 4 * w * h
    filt = np.frombuffer(raw[8:8 + 4 * w * h].tobytes(), dtype=np.float32).reshape(h, w)
    bias = np.frombuffer(raw[8 + 4 * w * h:].tobytes(), dtype=np.float32).reshape(h, w)
    return filt, bias


def model_arrays(model):
    return load_default_model() if model == "default" else synth.ccc_model()


def sample_image():
    """The reference's sample frame as a BGR image (720 x 540)."""
    from helpers import read_png
    img = np.ascontiguousarray(read_png(os.path.join(REF_WB, "alphasense.png")))
    assert img.shape == (540, 720, 3), img.shape
    return img


# ---- the oracle's answer to a case -----------------------------------------------------------------------------------------
def seen_image(O, form, f):
    """The BGR image the estimator sees: the debayered frame, or the colour frame in BGR order."""
    if form.startswith("bayer_"):
        return O.debayer(f, form)
    if form == "rgb8":
        return O.swap_rb(f)
    return np.ascontiguousarray(f)


Expected = collections.namedtuple("Expected", ["image", "estimate", "seen"])


def expected(O, method, params, form, f, occ=None):
    """The oracle's image and estimate of one frame.  estimate: grey_world {"q8", "sums"}, pca {"coeffs"}, simple {"ab"} (alpha
    and beta per channel), ccc {"track": raw x, raw y, x, y; "gains"} -- occ is the oracle.CCC object, whose filter state moves."""
    seen = seen_image(O, form, f)
    if method == "grey_world":
        img, sums, q8 = O.wb_grayworld(seen, params["wb_bright"], return_stats=True)
        est = dict(q8=[int(v) for v in q8], sums=[int(v) for v in sums])
    elif method == "pca":
        img, co = O.wb_pca(seen, return_coeffs=True)
        est = dict(coeffs=np.asarray(co, np.float32))
    elif method == "simple":
        img, ab = O.wb_simple(seen, params["wb_percentile"], return_coeffs=True)
        est = dict(ab=np.asarray(ab, np.float32))
    else:
        assert method == "ccc" and occ is not None
        occ.set_thresholds(params["wb_bright"], params["wb_dark"])
        img, info, gains = occ.balance(seen)
        est = dict(track=[int(v) for v in info], gains=np.asarray(gains, np.float32))
    return Expected(img, est, seen)


def same_floats(a, b):
    """Equal float32 bit patterns, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(both_nan | (a.view(np.uint32) == b.view(np.uint32))))


# ---- the statistics kernel's headroom (rip_stats.hip launch_stats, Bayer branch) ------------------------------------------------
HEADROOM_SIZE = (1024, 512)
HEADROOM_STATS_BLOCKS = 8
K_BLOCK = 256
MAX_PAIRS_PER_TASK = 128


def fast_stats_geometry(w, h, stats_blocks, n_frames):
    """launch_stats' arithmetic for a Bayer frame, restated: (col_waves, pairs_per_task, n_tasks, grid x)."""
    groups_, n_pairs = w // 4, h // 2
    col_waves = (groups_ + 63) // 64
    budget = max(8, stats_blocks // 8 * 8) * 4
    target = max(8, min(budget // (4 if n_frames == 1 else 8), budget // max(1, min(n_frames, 16))))
    pairs = max(2, (col_waves * n_pairs + target - 1) // target)
    pairs = min((pairs + 1) & ~1, MAX_PAIRS_PER_TASK)
    n_tasks = col_waves * ((n_pairs + pairs - 1) // pairs)
    task_blocks = (n_tasks + K_BLOCK // 64 - 1) // (K_BLOCK // 64)
    return col_waves, pairs, n_tasks, (task_blocks + 7) // 8 * 8


def task_sums(plane, col_waves, pairs_per_task):
    """Per wave task (a strip 256 pixels wide, pairs_per_task row pairs high) the sum of squares of a channel plane."""
    h, w = plane.shape
    sq = plane.astype(np.int64) ** 2
    out = []
    for y0 in range(0, h, 2 * pairs_per_task):
        for cw in range(col_waves):
            out.append(int(sq[y0:y0 + 2 * pairs_per_task, cw * 256:(cw + 1) * 256].sum()))
    return out


# ---- the reference's model and sample frame on the device ---------------------------------------------------------------------
REFERENCE_MODEL_FORMS = [("bgr8", (720, 540)), ("bayer_rggb8", (720, 540)), ("bayer_grbg8", (720, 540)), ("bayer_gbrg8", (720, 540)),
                         ("bayer_bggr8", (720, 540)), ("bgr8", (384, 240))]
# channel factors (B, G, R) that move the sample frame's illuminant; None is a black frame (an empty histogram inside a batch)
SAMPLE_TINTS = [(1.0, 1.0, 1.0), (0.8, 1.0, 1.15), None, (1.2, 0.9, 0.7), (0.6, 1.0, 0.9), (1.0, 0.7, 1.0), (0.9, 0.95, 0.5), (0.5, 0.8, 1.0)]


def reference_model_frames(form, size, n):
    """n different frames made of the reference's sample image: its tinted copies (frame 0 is the image itself, frame 2 black), cut
    down to `size` by taking every pixel nearest to the scaled position, as BGR or as a mosaic."""
    base = sample_image()
    w, h = size
    if (w, h) != (base.shape[1], base.shape[0]):
        ys = (np.arange(h) * base.shape[0]) // h
        xs = (np.arange(w) * base.shape[1]) // w
        base = base[ys][:, xs]
    out = []
    for i in range(n):
        tint = SAMPLE_TINTS[i % len(SAMPLE_TINTS)]
        if tint is None:
            bgr = np.zeros_like(base)
        else:
            k = 1.0 - 0.06 * (i // len(SAMPLE_TINTS))   # the second round of the list is darker: no two frames alike
            bgr = np.clip(np.rint(base.astype(np.float64) * (np.asarray(tint) * k)), 0, 255).astype(np.uint8)
        f = np.ascontiguousarray(bgr) if form == "bgr8" else synth.mosaic(bgr, form)
        f.setflags(write=False)
        out.append(f)
    return out
