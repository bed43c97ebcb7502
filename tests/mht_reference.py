"""Malvar-He-Cutler demosaic restated in numpy from the contract (PARITY.md, include/rip.h rip_set_debayer_method): the
expected image of the "mht" debayer method, for any Bayer pattern and 8- or 16-bit samples."""
import numpy as np

# phase (ry, rx) of the R sample in the 2 x 2 cell (parse_bayer, rip_plan.cpp)
PHASE = {"rggb": (0, 0), "grbg": (0, 1), "gbrg": (1, 0), "bggr": (1, 1)}

# The published filters, integer weights over 16, as {(dy, dx): weight} around the centre (the table in PARITY.md).
K_G = {(0, 0): 8, (0, -1): 4, (0, 1): 4, (-1, 0): 4, (1, 0): 4, (0, -2): -2, (0, 2): -2, (-2, 0): -2, (2, 0): -2}
K_ROW = {(0, 0): 10, (0, -1): 8, (0, 1): 8, (0, -2): -2, (0, 2): -2, (-2, 0): 1, (2, 0): 1,
         (-1, -1): -2, (-1, 1): -2, (1, -1): -2, (1, 1): -2}
K_COL = {(0, 0): 10, (-1, 0): 8, (1, 0): 8, (0, -2): 1, (0, 2): 1, (-2, 0): -2, (2, 0): -2,
         (-1, -1): -2, (-1, 1): -2, (1, -1): -2, (1, 1): -2}
K_DIAG = {(0, 0): 12, (0, -2): -3, (0, 2): -3, (-2, 0): -3, (2, 0): -3,
          (-1, -1): 4, (-1, 1): 4, (1, -1): 4, (1, 1): 4}
FILTERS = {"K_G": K_G, "K_row": K_ROW, "K_col": K_COL, "K_diag": K_DIAG}


def phase_of(encoding):
    """(ry, rx) of 'bayer_rggb8', 'bayer_bggr16', ... or of a bare pattern name."""
    name = encoding[len("bayer_"):] if encoding.startswith("bayer_") else encoding
    return PHASE[name.rstrip("0123456789")]


def reflect101(i, n):
    """Index of position i (-2 <= i <= n + 1) under reflect-101: -1 -> 1, -2 -> 2, n -> n - 2, n + 1 -> n - 3."""
    i = np.abs(np.asarray(i))
    return np.where(i >= n, 2 * n - 2 - i, i)


def filter_sum(frame, kernel):
    """S = sum of weight * sample over the kernel's taps at every pixel (int64), reflect-101 outside the frame."""
    h, w = frame.shape
    ys = reflect101(np.arange(-2, h + 2), h)
    xs = reflect101(np.arange(-2, w + 2), w)
    pad = frame.astype(np.int64)[np.ix_(ys, xs)]
    s = np.zeros((h, w), np.int64)
    for (dy, dx), wt in kernel.items():
        s += wt * pad[2 + dy:2 + dy + h, 2 + dx:2 + dx + w]
    return s


def round16(s, maxval):
    """clamp(round_half_even(s / 16), 0, maxval), in the integer form (s + 7 + ((s >> 4) & 1)) >> 4."""
    s = np.asarray(s, np.int64)
    return np.clip((s + 7 + ((s >> 4) & 1)) >> 4, 0, maxval)


def mht_reference(frame, encoding):
    """H x W Bayer frame (uint8 or uint16) -> H x W x 3 BGR of the same dtype, before any flip."""
    frame = np.asarray(frame)
    assert frame.ndim == 2 and frame.shape[0] >= 3 and frame.shape[1] >= 3
    maxval = 255 if frame.dtype == np.uint8 else 65535
    ry, rx = phase_of(encoding)
    h, w = frame.shape
    dy = ((np.arange(h) - ry) & 1)[:, None]
    dx = ((np.arange(w) - rx) & 1)[None, :]
    r_site, b_site = (dy == 0) & (dx == 0), (dy == 1) & (dx == 1)
    g_red_row, g_blue_row = (dy == 0) & (dx == 1), (dy == 1) & (dx == 0)
    c = frame.astype(np.int64)
    f = {name: round16(filter_sum(frame, k), maxval) for name, k in FILTERS.items()}
    b = np.select([b_site, r_site, g_red_row, g_blue_row], [c, f["K_diag"], f["K_col"], f["K_row"]])
    g = np.where(r_site | b_site, f["K_G"], c)
    r = np.select([r_site, b_site, g_red_row, g_blue_row], [c, f["K_diag"], f["K_row"], f["K_col"]])
    return np.stack([b, g, r], axis=2).astype(frame.dtype)


def flip(image, angle):
    """flip.cpp:40-52 on an H x W x C image: 90 = clockwise, 180, 270 = counter-clockwise; anything else unchanged."""
    if angle == 90:
        return np.ascontiguousarray(np.rot90(image, -1))
    if angle == 180:
        return np.ascontiguousarray(image[::-1, ::-1])
    if angle == 270:
        return np.ascontiguousarray(np.rot90(image, 1))
    return image
