"""The shapes at which the kernels of csrc/rip_area.hip can go wrong, shared by the kernel-on-the-host test (tests/test_resize_area.py)
and the GPU tests (tests/test_resize_area_gpu.py).  Importable without a GPU; nothing here looks at the library.

Sizes are (width, height).  The workgroup's output rectangle is TILE_W x TILE_H = 64 x 8 pixels (rip_area.hpp kAreaTileCols /
kAreaTileRows; tests/test_kernel_libraries.py checks the header still says so), one lane per output column, four waves that take the
rows w, w + 4 of the rectangle.  kind: "general" (tap lists), "whole" (block sums), "mean2" (the linear path's 2 x 2 kernel)."""
import collections

import numpy as np

TILE_W, TILE_H = 64, 8

Shape = collections.namedtuple("Shape", ["src", "dst", "kind", "what"])

TILE_EDGES = [
    Shape((95, 11), (63, 7), "general", "one below the rectangle on both axes, factor about 1.5"),
    Shape((96, 12), (64, 8), "general", "exactly one rectangle, factor 1.5"),
    Shape((98, 14), (65, 9), "general", "one above: a second rectangle of one column and one row"),
    Shape((200, 29), (133, 19), "general", "two rectangles and a ragged third on both axes"),
    Shape((195, 24), (65, 8), "whole", "whole 3 x 3, one column above a rectangle"),
    Shape((266, 38), (133, 19), "mean2", "2 x 2: the existing kernel"),
]
FACTORS = [
    Shape((41, 10), (40, 9), "general", "C = W + 1: two taps per output and dropped slivers"),
    Shape((23, 17), (23, 5), "general", "factor 1 on x"),
    Shape((23, 17), (5, 17), "general", "factor 1 on y"),
    Shape((45, 30), (30, 20), "general", "1.5 x 1.5"),
    Shape((30, 20), (20, 10), "general", "2 on y only"),
    Shape((30, 20), (15, 13), "general", "2 on x only"),
    Shape((30, 20), (15, 10), "mean2", "2 x 2"),
    Shape((201, 27), (67, 9), "whole", "3 x 3"),
    Shape((140, 20), (35, 10), "whole", "4 x 2"),
    Shape((30, 9), (10, 9), "whole", "3 x 1: a whole factor beside factor 1"),
    Shape((153, 128), (40, 30), "general", "3.825 x 4.27"),
    Shape((512, 256), (2, 1), "whole", "256 x 256: the largest block"),
    Shape((2051, 5), (1000, 5), "general", "a long strip, factor 2.051 beside factor 1"),
]
SHAPES = TILE_EDGES + FACTORS


def kernel_name(channels, kind):
    if kind == "mean2":
        return "resize_kernel<%d, true>" % channels
    return "area_reduce_kernel<%d, %s>" % (channels, "true" if kind == "whole" else "false")


def kind_of(src, dst):
    (sw, sh), (dw, dh) = src, dst
    if (sw, sh) == (dw, dh):
        return "identity"
    if (sw, sh) == (2 * dw, 2 * dh):
        return "mean2"
    return "whole" if sw % dw == 0 and sh % dh == 0 else "general"


assert all(kind_of(s.src, s.dst) == s.kind for s in SHAPES)


def tie_frame(channels):
    """A 24 x 8 frame -> 6 x 2 under whole 4 x 4: block sums 8, 24, 40, ... (quotients 0.5, 1.5, 2.5, ...: ties that round down to an
    even and up to an even value) and, in the second row of blocks, sums one off a tie on either side."""
    sums = [[8, 24, 40, 56, 72, 88], [7, 9, 23, 25, 4040, 4024]]
    f = np.zeros((8, 24, channels), np.uint8)
    for by, row in enumerate(sums):
        for bx, total in enumerate(row):
            for c in range(channels):
                t = total + 16 * c          # the channels differ by whole steps: the tie stays a tie
                block = np.full(16, t // 16, np.int64)
                block[:t % 16] += 1
                assert block.max() <= 255 and block.sum() == t
                f[4 * by:4 * by + 4, 4 * bx:4 * bx + 4, c] = np.roll(block, 3 * bx + c).reshape(4, 4)
    return f if channels == 3 else f[:, :, 0]


FUZZ_CASES = 40


def fuzz_case(seed):
    """A seeded draw: channels, source and target (sides up to 300, every factor from 1 to 256 can occur, no upscale), frames, and the
    destination's layout as indices (pitch 0..2, gap, base offset, format 0..9; the GPU test maps them to its own tables)."""
    rng = np.random.default_rng(77000 + seed)
    cn = int(rng.choice([1, 3]))
    dw, dh = (int(v) for v in rng.integers(1, 81, 2))
    roll = rng.random()
    if roll < 0.15:                                                  # whole factors
        sw, sh = dw * int(rng.integers(1, 5)), dh * int(rng.integers(1, 5))
    elif roll < 0.25:                                                # a whole factor on one axis only
        sw, sh = dw * int(rng.integers(1, 4)), int(rng.integers(dh, 301))
    elif roll < 0.32:                                                # a tiny target: large factors
        dw, dh = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        sw, sh = int(rng.integers(dw, 301)), int(rng.integers(dh, 301))
    else:
        sw, sh = int(rng.integers(dw, 301)), int(rng.integers(dh, 301))
    sw, sh = min(sw, 300, 256 * dw), min(sh, 300, 256 * dh)
    return dict(seed=seed, cn=cn, src=(sw, sh), dst=(dw, dh), n=int(rng.integers(1, 5)), pitch=int(rng.integers(3)), gap=bool(rng.integers(2)),
                base_off=bool(rng.integers(2)), fmt=int(rng.integers(10)))


def all_255(src, channels):
    w, h = src
    return np.full((h, w) if channels == 1 else (h, w, 3), 255, np.uint8)
