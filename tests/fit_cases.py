"""The shapes at which the kernels of librip_fit_hip.so (csrc/rip_fit.hip) can go wrong, shared by the kernels-on-the-host test
(tests/test_fit.py) and the GPU tests (tests/test_fit_gpu.py).  Importable without a GPU; nothing here looks at the library.

A case is a final image F of C x R pixels and `channels` channels, a window `roi` of it (None: all of F), a target (W, H) or None,
a fit mode, an interpolation and a pad colour (B, G, R).  Frames are seeded noise (``frames``)."""
import collections

import numpy as np

import fit_reference as FR

Case = collections.namedtuple("Case", ["channels", "size", "roi", "target", "fit", "interpolation", "pad", "n"])
PADS = ((114, 114, 114), (0, 255, 7), (201, 33, 90))     # the default, and two with three distinct bytes


def case(channels, size, roi, target, fit="stretch", interpolation="linear", pad=PADS[0], n=1):
    return Case(channels, tuple(size), None if roi is None else tuple(roi), None if target is None else tuple(target), fit, interpolation, tuple(pad), n)


def case_id(c):
    return "%dch-%dx%d-roi%s-to%s-%s-%s" % (c.channels, c.size[0], c.size[1], "x".join(map(str, c.roi)) if c.roi else "none",
                                           "x".join(map(str, c.target)) if c.target else "none", c.fit, c.interpolation)


def frames(c, seed=0):
    """c.n frames of uniform noise.  Fresh array, deterministic."""
    (w, h), cn = c.size, c.channels
    rng = np.random.default_rng(9000 + seed + 7 * w + 13 * h + cn)
    return rng.integers(0, 256, (c.n, h, w) if cn == 1 else (c.n, h, w, 3), dtype=np.uint8)


# window size -> target size of each path: (interpolation, (ws, hs), (W, H))
PATHS = {"linear": ("linear", (11, 7), (7, 5)), "mean2": ("linear", (10, 6), (5, 3)), "whole": ("area", (12, 8), (4, 2)),
         "taps": ("area", (7, 7), (5, 5)), "copy": ("area", (9, 4), (9, 4))}
ORIGIN_XS, ORIGIN_YS = (0, 1, 2, 3, 5), (0, 1)


def origin_cases():
    """The window's origin against dword alignment: with 3 channels xs = 0, 1, 2, 3 start at byte phases 0, 3, 2, 1 and 5 at phase 3
    of the next dword; with one channel the phase is xs & 3.  ys = 1: F ends with the window (its last column and row are the
    window's); ys = 0: F goes on for 3 columns and 2 rows, which must not be seen."""
    out = []
    for path, (interp, (ws, hs), target) in sorted(PATHS.items()):
        for cn in (1, 3):
            for xs in ORIGIN_XS:
                for ys in ORIGIN_YS:
                    size = (xs + ws, ys + hs) if ys else (xs + ws + 3, hs + 2)
                    out.append(case(cn, size, (xs, ys, ws, hs), target, "stretch", interp))
    return out


LANE_WIDTHS = (1, 3, 4, 5, 1021, 1024, 1025, 1027)   # rip_resize.hpp: 4 pixels per lane, 1024 per workgroup


def lane_cases():
    """Picture widths around a lane and a workgroup of the linear and 2 x 2 kernels, 5 rows, from a window at xs = 1."""
    out = []
    for cn in (1, 3):
        for w in LANE_WIDTHS:
            ws = max(3, (w * 17 + 5) // 10)                 # about 1.7 x: a non-integer downscale
            out.append(case(cn, (ws + 2, 9), (1, 1, ws, 8), (w, 5)))
            out.append(case(cn, (2 * w + 1, 11), (1, 0, 2 * w, 10), (w, 5)))
    return out


def tile_cases():
    """63, 64 and 65 columns by 7, 8 and 9 rows of the area kernels (rip_area.hpp: a workgroup owns 64 x 8 pixels), from a window at
    xs = 1: whole factors 3 x 4 and tap lists at about 1.5."""
    out = []
    for cn in (1, 3):
        for w in (63, 64, 65):
            for h in (7, 8, 9):
                out.append(case(cn, (3 * w + 2, 4 * h + 1), (1, 1, 3 * w, 4 * h), (w, h), "stretch", "area"))
                ws, hs = (3 * w + 1) // 2, (3 * h + 1) // 2
                out.append(case(cn, (ws + 1, hs + 2), (1, 2, ws, hs), (w, h), "stretch", "area"))
    return out


def band_cases():
    """Letterboxes: left = 0, 1, 2, 3, 5 with side bands only, an odd remainder (the right band one wider than the left), top and
    bottom bands only, a picture of one row and of one column, and a crop; three pad colours."""
    out = []
    for cn in (1, 3):
        for i, left in enumerate((1, 2, 3, 5)):
            out.append(case(cn, (16, 16), None, (8 + 2 * left, 8), "letterbox", "linear", PADS[i % 3]))        # the 2 x 2 mean of all of F
            out.append(case(cn, (19, 17), (2, 1, 16, 16), (8 + 2 * left + 1, 8), "letterbox", "area", PADS[(i + 1) % 3]))  # odd remainder, a window
        out.append(case(cn, (8, 8), None, (14, 8), "letterbox", "linear", PADS[1]))                          # a copy of F between two bands
        out.append(case(cn, (21, 9), None, (13, 11), "letterbox", "linear", PADS[2]))                        # top and bottom only, left = 0
        out.append(case(cn, (21, 9), (1, 0, 20, 9), (13, 12), "letterbox", "area", PADS[1]))                 # the same with a window and an odd remainder
        out.append(case(cn, (403, 5), (3, 1, 400, 3), (64, 64), "letterbox", "linear", PADS[2]))             # a picture of one row
        out.append(case(cn, (5, 403), (1, 3, 3, 400), (64, 64), "letterbox", "area", PADS[1]))               # a picture of one column
        out.append(case(cn, (1031, 6), None, (1029, 9), "letterbox", "linear", PADS[1]))                     # bands across a workgroup boundary
        out.append(case(cn, (37, 21), (0, 0, 37, 20), (10, 10), "crop", "area"))
        out.append(case(cn, (37, 21), None, (10, 10), "crop", "linear"))
        out.append(case(cn, (30, 20), (3, 2, 13, 7), None))                                                   # no target: the window itself
    return out


def kernel_cases():
    return origin_cases() + lane_cases() + tile_cases() + band_cases()


def geometry(c):
    return FR.geometry(c.size[0], c.size[1], c.roi, c.target, c.fit)


def kernel_of(c):
    """The resize kernel a case runs (fit_reference.kernel_name) and whether the pad kernel follows."""
    src, dst, delivered = geometry(c)
    windowed = src != (0, 0) + c.size
    return FR.kernel_name(c.channels, FR.rule(src[2:], dst[2:], c.interpolation), windowed), dst[2:] != delivered
