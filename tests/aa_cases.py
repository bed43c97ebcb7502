"""The shapes at which the antialiased resize (csrc/rip_aa.hip, "linear_aa" / "cubic_aa") can go wrong, shared by the CPU tests
(tests/test_resize_aa.py: the pin against torch, the kernels run on the host) and the GPU tests (tests/test_resize_aa_gpu.py).

Importable without a GPU; nothing here looks at the library.  Sizes are (w, h)."""
import collections

import numpy as np

FILTER_NAMES = ("linear_aa", "cubic_aa")
TILE_W = 64
MAX_FACTOR = 64

Shape = collections.namedtuple("Shape", ["src", "dst", "why"])

# A workgroup owns 64 output columns x TH output rows (TH = 8 for all of these): targets 63 / 64 / 65 / 129 wide and 7 / 8 / 9 / 17 high
# are one tile less a pixel, exactly one, one more, and two more.
SHAPES = (
    Shape((200, 136), (67, 45), "two column tiles, six row tiles, factor 3"),
    Shape((150, 111), (65, 9), "a second tile of one column and of one row"),
    Shape((190, 40), (63, 7), "one ragged tile"),
    Shape((200, 50), (64, 8), "exactly one tile"),
    Shape((300, 60), (129, 17), "three column and three row tiles"),
    Shape((37, 29), (80, 61), "an upscale on both axes"),
    Shape((100, 60), (100, 25), "the horizontal pass skipped"),
    Shape((100, 60), (41, 60), "the vertical pass skipped"),
    Shape((60, 25), (60, 40), "the horizontal pass skipped, rows enlarged"),
    Shape((1, 1), (5, 7), "a one-pixel source"),
    Shape((40, 30), (1, 30), "a one-pixel-wide target, rows unchanged"),
    Shape((90, 31), (45, 62), "columns halved, rows doubled"),
    Shape((64, 64), (32, 32), "exactly half: no 2 x 2 special case under these names"),
)

# (filter, channels, src, dst): a tall narrow frame for each tile height the host chooses (cubic_aa on 3 channels at a factor of 64:
# two output rows read 4 * 64 + 1 + 64 = 321 source rows, 61 632 bytes of LDS)
TILE_HEIGHT_SHAPES = (
    ("cubic_aa", 3, (8, 1280), (8, 20)),
    ("cubic_aa", 3, (8, 800), (8, 20)),
    ("linear_aa", 3, (8, 1280), (8, 20)),
    ("cubic_aa", 3, (8, 400), (8, 20)),
    ("cubic_aa", 1, (8, 1280), (8, 20)),
)


def kernel_name(channels, window):
    return "aa_kernel<%d, %s>" % (channels, "true" if window else "false")


def noise(w, h, n, cn, seed=0):
    rng = np.random.default_rng(7000 + seed)
    return rng.integers(0, 256, (n, h, w) if cn == 1 else (n, h, w, cn), dtype=np.uint8)


def binary_noise(w, h, n, cn, seed=0):
    """0 / 255 noise: the cubic filter's negative lobes leave [0, 255] on both sides."""
    rng = np.random.default_rng(7100 + seed)
    return (rng.integers(0, 2, (n, h, w) if cn == 1 else (n, h, w, cn), dtype=np.uint8) * 255).astype(np.uint8)


# ---- the pin against torch: 558 seeded draws and 10 fixed pairs under both channel counts, 578 per filter ----------------------------
PinCase = collections.namedtuple("PinCase", ["src", "dst", "channels", "binary", "channels_last"])
FIXED_PAIRS = (((4096, 6), (16, 3)), ((5, 4096), (2, 16)), ((16384, 4), (64, 2)), ((3, 16384), (3, 64)), ((1000, 999), (999, 1000)), ((640, 7), (641, 7)),
               ((9, 640), (4, 641)), ((1, 1), (5, 7)), ((50, 37), (50, 20)), ((50, 37), (23, 37)))


def pin_cases():
    rng = np.random.default_rng(578)
    out = []
    while len(out) < 558:
        sw, sh, dw, dh = (int(v) for v in rng.integers(1, 201, 4))
        keep = int(rng.integers(0, 8))
        if keep == 0:
            dw = sw
        elif keep == 1:
            dh = sh
        cn, binary, cl = (1, 3)[int(rng.integers(0, 2))], bool(rng.integers(0, 4) == 0), bool(rng.integers(0, 2))
        if (dw, dh) == (1, 1):          # torch dies with an internal assert on a 3-channel target of exactly 1 x 1: the one thing left out
            continue
        out.append(PinCase((sw, sh), (dw, dh), cn, binary, cl))
    for k, (src, dst) in enumerate(FIXED_PAIRS):
        for cn in (1, 3):
            out.append(PinCase(src, dst, cn, False, bool((k + cn) % 2)))
    return out


# ---- the seeded fuzz of the GPU tests ---------------------------------------------------------------------------------------------------
FUZZ_CASES = 40


def fuzz_case(seed):
    rng = np.random.default_rng(9100 + seed)
    sw, sh = int(rng.integers(1, 260)), int(rng.integers(1, 200))
    pick = lambda s: max(1, -(-s // MAX_FACTOR), int(s * float(rng.choice([0.11, 0.3, 0.5, 0.77, 1.0, 1.4, 2.2])) + int(rng.integers(-1, 2))))
    dw, dh = min(pick(sw), 300), min(pick(sh), 300)
    if (dw, dh) == (sw, sh):
        dw += 1
    return dict(src=(sw, sh), dst=(dw, dh), cn=(1, 3)[int(rng.integers(0, 2))], n=int(rng.integers(1, 4)), name=FILTER_NAMES[int(rng.integers(0, 2))],
                fmt=int(rng.integers(0, 64)), pitch=int(rng.integers(0, 3)), gap=bool(rng.integers(0, 2)), base_off=bool(rng.integers(0, 2)))
