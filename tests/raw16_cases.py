"""Frames and seeded cases of tests/test_raw16_gpu.py: pure functions of the seed, so that tests/test_raw16.py can check on the
CPU that the fuzz generator only produces valid combinations (no case is skipped or filtered out after generation) and reaches
what it is there for.  The stage configuration comes from ``random_case`` of tests/test_fuzz_gpu.py."""
import os

import numpy as np

from helpers import LAYOUTS, cfg
from raw_image_pipeline_amd import synth
from test_fuzz_gpu import random_case

N_FUZZ = int(os.environ.get("RIP_FUZZ_CASES", "40"))   # the variable of tests/test_fuzz_gpu.py: raise it for a soak run

NAMES = ["rggb", "bggr", "gbrg", "grbg"]
METHODS = ["bilinear", "mht"]
ANGLES = [0, 90, 180, 270]
FLIPS = ["off", 0, 90, 180, 270]
# the ranges of the all-values test: full scale, identity, one step, 10 bits, 10 bits with a black level, 12 bits with one,
# exact multiples of 256, a range of one value near the bottom and at the top, and one with nothing round about it
RANGES = [(0, 65535), (0, 255), (0, 1), (0, 1023), (64, 1023), (256, 4095), (0, 65280), (1000, 1001), (65534, 65535), (12345, 54321)]
# on and around the edges of the 64 x 32 tiles (width, height)
EDGE_SIZES = [(3, 3), (5, 7), (63, 31), (64, 32), (65, 33), (130, 70), (257, 129)]
BATCHES = [1, 3, 4, 5, 9, 17]   # 4 frames per workgroup visit
FUZZ_SEED = 16000


def enc8(name):
    return "bayer_%s8" % name


def enc16(name):
    return "bayer_%s16" % name


def gen_frame16(w, h, name, seed, black, white, kind="scene", tint=(0.70, 1.00, 0.55)):
    """A uint16 Bayer frame for the range (black, white).  'random': every sample uniform over all 65536 values.  Otherwise the
    8-bit synthetic frame of that kind stretched over the range, with sensor noise of about 1 % of it, one block of samples at
    or below the black level and one at or above the white level -- data that lies outside the range on both sides."""
    rng = np.random.default_rng(50000 + seed)
    if kind == "random":
        return rng.integers(0, 65536, (h, w)).astype(np.uint16)
    r = white - black
    f = black + synth.gen_frame(w, h, enc8(name), seed=seed, kind=kind, tint=tint).astype(np.int64) * r // 255
    f += rng.integers(-(r // 100) - 1, r // 100 + 2, (h, w))
    bh, bw = max(1, h // 5), max(1, w // 5)
    f[:bh, w - bw:] = rng.integers(0, black + 1, (bh, bw))
    f[h - bh:, :bw] = rng.integers(white, 65536, (bh, bw))
    return np.clip(f, 0, 65535).astype(np.uint16)


def random_range(rng):
    kind = int(rng.integers(0, 4))
    if kind == 0:   # a sensor's bit depth with a black level
        bits = int(rng.choice([8, 10, 12, 14, 16]))
        return int(rng.integers(0, (1 << bits) // 8)), (1 << bits) - 1 - int(rng.integers(0, 3))
    if kind == 1:   # narrow
        black = int(rng.integers(0, 65000))
        return black, black + int(rng.integers(1, 300))
    black = int(rng.integers(0, 65535))
    return black, int(rng.integers(black + 1, 65536))


def fuzz_case(seed):
    """Every combination this returns is valid for the library and for the oracle: nothing is rejected afterwards."""
    rng = np.random.default_rng(FUZZ_SEED + seed)
    _, _, _, kind, c = random_case(rng)
    name = NAMES[int(rng.integers(0, 4))]
    method = METHODS[seed % 2]
    black, white = random_range(rng)
    if rng.random() < 0.5:
        w, h = EDGE_SIZES[int(rng.integers(0, len(EDGE_SIZES)))]
        w, h = w + int(rng.integers(0, 3)), h + int(rng.integers(0, 3))
    else:
        w, h = 4 * int(rng.integers(8, 90)), 2 * int(rng.integers(8, 70))
    flip = FLIPS[int(rng.integers(0, len(FLIPS)))]
    if min(w, h) < 9:   # nothing else in the suite runs the later stages that small: demosaic, narrowing and flip only
        c = cfg()
    c["flip"] = flip != "off"
    c["flip_angle"] = 0 if flip == "off" else int(flip)
    ow, oh = (h, w) if flip in (90, 270) else (w, h)
    c["cam"] = synth.camera_model(ow, oh)
    interior = w >= 200 and h >= 100
    n = int(rng.choice([v for v in BATCHES if v >= 5] if interior else BATCHES))
    layout = LAYOUTS[int(rng.integers(0, len(LAYOUTS)))]
    tint = (float(rng.uniform(0.5, 1)), 1.0, float(rng.uniform(0.5, 1)))
    if rng.random() < 0.25:
        kind = "random"
    return dict(seed=seed, w=w, h=h, name=name, method=method, black=black, white=white, kind=kind, c=c, flip=flip, n=n, layout=layout,
                tap=seed % 4 < 2, tint=tint, layout_seed=int(rng.integers(0, 1 << 30)))


def describe(case):
    c = case["c"]
    return "seed %d: %dx%d %s %s range (%d, %d) n %d %s %s" % (
        case["seed"], case["w"], case["h"], case["name"], case["method"], case["black"], case["white"], case["n"], case["layout"],
        {k: v for k, v in c.items() if k not in ("cam", "cc_matrix")})
