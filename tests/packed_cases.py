"""Frames and seeded cases of tests/test_packed_gpu.py: pure functions of the seed, so that tests/test_packed.py can check on
the CPU that the fuzz generator only produces valid combinations and reaches what it is there for.  The stage configuration
comes from ``random_case`` of tests/test_fuzz_gpu.py, the frames from tests/raw16_cases.py (clipped to the format)."""
import numpy as np

import packed_reference as R
import raw16_cases as G
from helpers import LAYOUTS as BATCH_LAYOUTS
from helpers import batch_geometry, cfg
from raw_image_pipeline_amd import synth
from test_fuzz_gpu import random_case

N_FUZZ = G.N_FUZZ   # RIP_FUZZ_CASES, default 40
FUZZ_SEED = 26000
# the kernel's tile is 64 x 32 pixels with a 2-px halo: interior tiles exist from 130 x 66 on
TILE_W, TILE_H = 64, 32
# widths whose interior tile spans meet the dword-alignment cases of both bit depths, and one frame of 3 x 3 tiles and more
INTERIOR_SIZES = [(64, 66), (66, 66), (128, 66), (130, 66), (192, 70), (196, 70), (200, 100)]
RANGES = {10: [None, (0, 1023), (64, 1023), (0, 4095)], 12: [None, (0, 4095), (256, 4095), (100, 60000)]}


def sizes(layout):
    """EDGE_SIZES of the 16-bit tests and the interior sizes, each width moved to the nearest one the layout allows."""
    return sorted({(R.allowed_width(w, layout), h) for w, h in G.EDGE_SIZES + INTERIOR_SIZES})


def effective_range(layout, rng_range):
    return R.natural_range(layout) if rng_range is None else rng_range


def gen_samples(w, h, name, seed, layout, black, white, kind="scene", tint=(0.70, 1.00, 0.55)):
    """uint16 samples below 2^B: the frames of raw16_cases.gen_frame16 for the part of the range the format can hold, clipped to
    it ('random': uniform over all 2^B values)."""
    top = (1 << R.BITS[layout]) - 1
    if kind == "random":
        return np.random.default_rng(70000 + seed).integers(0, top + 1, (h, w)).astype(np.uint16)
    return np.minimum(G.gen_frame16(w, h, name, seed, min(black, top - 1), min(white, top), kind=kind, tint=tint), top).astype(np.uint16)


def has_interior_tiles(w, h):
    return w >= 2 * TILE_W + 2 and h >= 2 * TILE_H + 2


def fuzz_case(seed):
    """Every combination this returns is valid for the library and for the oracle: nothing is rejected afterwards."""
    rng = np.random.default_rng(FUZZ_SEED + seed)
    _, _, _, kind, c = random_case(rng)
    layout = R.LAYOUTS[seed % 4]
    method = G.METHODS[(seed // 4) % 2]
    name = G.NAMES[int(rng.integers(0, 4))]
    ranges = RANGES[R.BITS[layout]]
    rng_range = ranges[int(rng.integers(0, len(ranges)))]
    if rng.random() < 0.4:
        w, h = G.EDGE_SIZES[int(rng.integers(0, len(G.EDGE_SIZES)))]
        w, h = w + int(rng.integers(0, 3)), h + int(rng.integers(0, 3))
    else:
        w, h = int(rng.integers(130, 330)), int(rng.integers(66, 140))
        if rng.random() < 0.6:   # a sensor's width: rows of whole dwords at both bit depths, so that tight batches are aligned
            w = (w + 15) // 16 * 16
    w = R.allowed_width(w, layout)
    flip = G.FLIPS[int(rng.integers(0, len(G.FLIPS)))]
    if min(w, h) < 9:   # nothing else in the suite runs the later stages that small
        c = cfg()
    c["flip"] = flip != "off"
    c["flip_angle"] = 0 if flip == "off" else int(flip)
    ow, oh = (h, w) if flip in (90, 270) else (w, h)
    c["cam"] = synth.camera_model(ow, oh)
    n = int(rng.choice([v for v in G.BATCHES if v >= 5] if has_interior_tiles(w, h) else G.BATCHES))
    batch_layout = BATCH_LAYOUTS[int(rng.integers(0, len(BATCH_LAYOUTS)))]
    layout_seed = int(rng.integers(0, 1 << 30))
    # the geometry tests/helpers.py device_batch will draw from the same seed: aligned batches take the dword path in their
    # interior tiles, every other one the byte path everywhere
    offset, pitch, stride = batch_geometry(batch_layout, R.row_bytes(w, layout), h, np.random.default_rng(layout_seed))
    aligned = offset % 4 == 0 and pitch % 4 == 0 and stride % 4 == 0
    tint = (float(rng.uniform(0.5, 1)), 1.0, float(rng.uniform(0.5, 1)))
    if rng.random() < 0.25:
        kind = "random"
    return dict(seed=seed, w=w, h=h, name=name, layout=layout, method=method, range=rng_range, kind=kind, c=c, flip=flip, n=n,
                batch_layout=batch_layout, layout_seed=layout_seed, tap=seed % 3 == 0, tint=tint,
                path="interior" if aligned and has_interior_tiles(w, h) else "byte")


def describe(case):
    c = case["c"]
    return "seed %d: %dx%d %s %s %s range %s n %d %s (%s path) %s" % (
        case["seed"], case["w"], case["h"], case["name"], case["layout"], case["method"], case["range"], case["n"], case["batch_layout"],
        case["path"], {k: v for k, v in c.items() if k not in ("cam", "cc_matrix")})
