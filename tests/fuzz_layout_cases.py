"""Case generators of tests/test_fuzz_layout_gpu.py: pure functions of the seed, so that tests/test_fuzz_layout_cases.py can
check on the CPU that the default case counts reach what the fuzz is there for (every batch layout, the frames-per-visit
boundaries of the kernels, the tile edges of the MHT kernel, the footprint walk) before any GPU time is spent.

The stage configuration comes from ``random_case`` of tests/test_fuzz_gpu.py; size, batch length and layout are replaced."""
import os

import numpy as np

from helpers import LAYOUTS, cfg
from raw_image_pipeline_amd import synth
from test_fuzz_gpu import PATTERNS, random_case

N_CASES = int(os.environ.get("RIP_FUZZ_CASES", "60"))   # the variable of tests/test_fuzz_gpu.py: RIP_FUZZ_CASES=600 for a soak run
N_MHT = N_CASES
N_LAYOUT = N_CASES
N_FOOTPRINT = max(8, N_CASES // 2)

FLIPS = ["off", 0, 90, 180, 270]

# ---- family 1: MHT ------------------------------------------------------------------------------------------------------
# around the 64 x 32 tiles of demosaic_mht_tile_kernel and its 2-px halo: sizes below one tile, and one, two, three tiles +- a few
MHT_WIDTH_CLASSES = [range(3, 10), range(60, 69), range(124, 133), range(188, 197)]
MHT_HEIGHT_CLASSES = [range(3, 8), range(29, 36), range(61, 68), range(93, 100)]
MHT_BATCHES = [1, 4, 5, 7, 8, 9, 13, 17]   # 4 frames per workgroup visit: one group, two even, two and three uneven, 4 + 1
MHT_SEED = 13000


def _set_flip(c, flip, w, h):
    """Flip state 'off' or an angle; the camera of the configuration follows the post-flip size."""
    c["flip"] = flip != "off"
    c["flip_angle"] = 0 if flip == "off" else int(flip)
    ow, oh = (h, w) if flip in (90, 270) else (w, h)
    c["cam"] = synth.camera_model(ow, oh)
    return c


def mht_case(seed):
    rng = np.random.default_rng(MHT_SEED + seed)
    _, _, pattern, kind, c = random_case(rng)
    edge = bool(rng.random() < 0.5)
    if edge:
        w = int(rng.choice(np.concatenate([np.asarray(r) for r in MHT_WIDTH_CLASSES])))
        h = int(rng.choice(np.concatenate([np.asarray(r) for r in MHT_HEIGHT_CLASSES])))
    else:
        kw, kh = int(rng.integers(8, 101)), int(rng.integers(8, 81))
        if rng.random() < 0.25 and kw % 4 == 0:   # cols * 3 % 16 != 0: the handle's MHT image gets padded rows
            kw += 1
        w, h = 4 * kw, 2 * kh
    flip = FLIPS[int(rng.integers(0, len(FLIPS)))]
    if min(w, h) < 9:   # nothing else in the suite runs the later stages that small: demosaic and flip only
        c = cfg()
    _set_flip(c, flip, w, h)
    interior = w >= 200 and h >= 100   # sizes with tiles whose halo lies inside the frame (the register prefetch)
    n = int(rng.choice([v for v in MHT_BATCHES if v >= 5] if interior else MHT_BATCHES))
    layout = LAYOUTS[int(rng.integers(0, len(LAYOUTS)))]
    tint = (float(rng.uniform(0.5, 1)), 1.0, float(rng.uniform(0.5, 1)))
    return dict(seed=seed, w=w, h=h, pattern=pattern, kind=kind, c=c, flip=flip, n=n, layout=layout, tap=seed % 2 == 0, tint=tint,
                edge=edge, layout_seed=int(rng.integers(0, 1 << 30)))


# ---- family 2: bilinear Bayer, colour and mono input -----------------------------------------------------------------------
LAYOUT_ENCODINGS = PATTERNS + ["bgr8", "rgb8", "mono8"]
# frames per workgroup visit: 16 in the Lab chain and the fused remap, 6 and 2 in the other chains, 4 to 12 in the remap
LAYOUT_BATCHES = [1, 2, 5, 6, 7, 12, 13, 16, 17, 33]
LAYOUT_SEED = 14000
LAYOUT_PIXEL_CAP = 800000   # n * rows * cols: the oracle does about 3 Mpx/s with every stage on, and the file should cost about
                            # twice tests/test_fuzz_gpu.py


def layout_case(seed):
    rng = np.random.default_rng(LAYOUT_SEED + seed)
    _, _, _, kind, c = random_case(rng)
    # stratified, so that every encoding meets every layout and every batch length within 70 cases whatever the seed base
    encoding = LAYOUT_ENCODINGS[seed % len(LAYOUT_ENCODINGS)]
    layout = LAYOUTS[(seed // len(LAYOUT_ENCODINGS)) % len(LAYOUTS)]
    n = LAYOUT_BATCHES[seed % len(LAYOUT_BATCHES)]
    max_w, max_h = (200, 120) if n == 33 else (400, 300)
    if rng.random() < 0.7:
        w, h = 4 * int(rng.integers(8, max_w // 4 + 1)), 2 * int(rng.integers(8, max_h // 2 + 1))
        while n * w * h > LAYOUT_PIXEL_CAP:
            h -= 2
    else:
        w, h = int(rng.integers(9, max_w + 1)), int(rng.integers(9, max_h + 1))
        while n * w * h > LAYOUT_PIXEL_CAP:
            h -= 1
    flip = FLIPS[int(rng.integers(0, len(FLIPS)))]
    _set_flip(c, flip, w, h)
    if encoding == "mono8":
        c.update(vig=False)   # cvtColor(BGR2Lab) asserts on one channel (test_error_behaviour)
    return dict(seed=seed, w=w, h=h, encoding=encoding, kind=kind, c=c, flip=flip, n=n, layout=layout,
                layout_seed=int(rng.integers(0, 1 << 30)))


# ---- family 3: the footprint walk -----------------------------------------------------------------------------------------
FOOTPRINT_BATCHES = [1, 3, 16, 17, 20]   # 16 frames per visit in the Lab chain
FOOTPRINT_LAYOUTS = ["tight", "pitch16", "frame_gap"]   # dword-aligned: the others send the chain to the generic kernels (no item list)
FOOTPRINT_SEED = 15000


def moved_camera(w, h, dx, dy):
    """synth.camera_model with the principal point moved by (dx * w, dy * h)."""
    cam = synth.camera_model(w, h)
    K = list(cam["K"])
    K[2] += dx * w
    K[5] += dy * h
    P = list(cam["P"])
    P[2], P[6] = K[2], K[5]
    cam["K"], cam["P"] = K, P
    return cam


def footprint_case(seed):
    rng = np.random.default_rng(FOOTPRINT_SEED + seed)
    _, _, pattern, kind, c = random_case(rng)
    w, h = 4 * int(rng.integers(50, 251)), 2 * int(rng.integers(50, 201))
    flip = ["off", 0, 180][int(rng.integers(0, 3))]
    _set_flip(c, flip, w, h)
    c["cam"] = moved_camera(w, h, float(rng.uniform(-0.1, 0.1)), float(rng.uniform(-0.1, 0.1)))
    c["undistort"] = True
    c["balance"], c["fov_scale"] = float(rng.uniform(0, 0.6)), float(rng.uniform(0.7, 1.5))
    if not (c["vig"] or c["ce"]):   # a stage the remap's tiles do not fuse: the chain runs as a kernel of its own
        c["vig" if rng.random() < 0.5 else "ce"] = True
    n = int(rng.choice(FOOTPRINT_BATCHES))
    layout = FOOTPRINT_LAYOUTS[int(rng.integers(0, len(FOOTPRINT_LAYOUTS)))]
    return dict(seed=seed, w=w, h=h, pattern=pattern, kind=kind, c=c, flip=flip, n=n, layout=layout,
                layout_seed=int(rng.integers(0, 1 << 30)))


def describe(case):
    c = case["c"]
    return "seed %d: %dx%d %s n %d %s %s" % (case["seed"], case["w"], case["h"], case.get("pattern", case.get("encoding")), case["n"], case["layout"],
                                             {k: v for k, v in c.items() if k not in ("cam", "cc_matrix")})
