"""The shapes, contents and layouts the CLAHE tests share (tests/test_clahe.py on the CPU, tests/test_clahe_gpu.py on the GPU): the
smallest at which each piece of csrc/rip_clahe_dev.hpp can go wrong.  Importable without a GPU; nothing here looks at the library."""
import collections

import numpy as np

# (width, height), (tiles_x, tiles_y): what the shape is there for
SHAPES = [
    ((64, 48), (8, 8)),       # both axes divide: E = P
    ((67, 45), (8, 8)),       # neither divides
    ((64, 45), (8, 8)),       # the width divides and is extended by a full tiles_x all the same
    ((67, 48), (8, 8)),       # the height divides ...
    ((40, 30), (1, 1)),       # one tile: no blend
    ((32, 32), (16, 16)),     # two-pixel tiles, the smallest accepted
    ((50, 41), (3, 5)),
    ((70, 9), (16, 1)),
    ((1100, 70), (4, 2)),     # wider than one pass of a workgroup (256 lanes x 4 pixels)
]
# A = 105 000 pixels per tile: a bin count passes 65 535
LARGE_SHAPE = ((700, 300), (2, 1))
CLIPS = (0.0, 0.01, 3.0, 40.0, 1e9)      # none; cl = 1; usual; mild; above every count
CONTENTS = ("flat", "noise01", "gradient", "random")


def picture(content, height, width, seed=0):
    """uint8 [height, width]."""
    rng = np.random.default_rng(seed)
    if content == "flat":
        return np.full((height, width), 100 + seed % 100, np.uint8)
    if content == "noise01":       # saturated: only the bins 0 and 255
        return (rng.integers(0, 2, (height, width)) * 255).astype(np.uint8)
    if content == "gradient":
        y, x = np.mgrid[0:height, 0:width]
        return ((x * 3 + y * 5 + seed) % 256).astype(np.uint8)
    assert content == "random"
    return rng.integers(0, 256, (height, width), dtype=np.uint8)


# ---- the kernels run on the host (tests/cpp/clahe_kernel_host.cpp) and the destinations of the GPU tests -------------------------
# dst row padding, dst offset, frame gap
LAYOUTS = ((0, 0, 0), (16 - 3, 0, 0), (1, 0, 5), (0, 1, 0), (3, 2, 7), (2, 3, 1))
HostCase = collections.namedtuple("HostCase", "height width tiles_x tiles_y frames in_place pad offset gap clip content")


def host_cases():
    out = []
    k = 0
    for (w, h), (tx, ty) in SHAPES:
        for in_place in (0, 1):
            pad, off, gap = LAYOUTS[k % len(LAYOUTS)]
            out.append(HostCase(h, w, tx, ty, (1, 3, 2)[k % 3], in_place, pad, off, gap, CLIPS[k % len(CLIPS)], CONTENTS[k % len(CONTENTS)]))
            k += 1
    for layout in LAYOUTS:                       # every layout on one odd shape, both ways
        for in_place in (0, 1):
            out.append(HostCase(45, 67, 8, 8, 2, in_place, *layout, 3.0, "random"))
    for clip in CLIPS:                           # every clip on every content
        for content in CONTENTS:
            out.append(HostCase(45, 67, 4, 3, 1, k % 2, 1, 1, 0, clip, content))
            k += 1
    (w, h), (tx, ty) = LARGE_SHAPE
    out.append(HostCase(h, w, tx, ty, 1, 0, 0, 0, 0, 3.0, "flat"))
    out.append(HostCase(h, w, tx, ty, 1, 1, 1, 3, 0, 40.0, "random"))
    return out


# ---- the seeded fuzz -----------------------------------------------------------------------------------------------------------
FUZZ_CASES = 40


def fuzz_case(seed):
    """One configuration: a picture size, tiles the size accepts, a clip, a content, a layout, a batch and the path."""
    rng = np.random.default_rng(1000 + seed)
    tx, ty = int(rng.integers(1, 17)), int(rng.integers(1, 17))
    w, h = int(rng.integers(2 * tx, 2 * tx + 120)), int(rng.integers(2 * ty, 2 * ty + 90))
    clip = float(CLIPS[int(rng.integers(len(CLIPS)))]) if seed % 3 else float(rng.uniform(0.0, 8.0))
    return dict(width=w, height=h, tiles=(tx, ty), clip=clip, content=CONTENTS[int(rng.integers(len(CONTENTS)))],
                layout=LAYOUTS[int(rng.integers(len(LAYOUTS)))], frames=(1, 3, 5)[int(rng.integers(3))], resized=bool(seed % 2))
