"""The YUV 4:2:0 output formats (include/rip.h rip_set_output_yuv_matrix; PARITY.md "Output formats: YUV 4:2:0") restated in numpy
int64, from the definition and not from the kernel: per pixel Y = (yb B + yg G + yr R + (yoff << 15) + 16384) >> 15, per 2 x 2 block
with the plain channel sums SB, SG, SR: Cb = min(255, (cbb SB + cbg SG + cbr SR + (128 << 17) + 65536) >> 17), Cr alike.

Importable without a GPU."""
import numpy as np

FORMATS = ("nv12", "i420")
# name: (yoff, (yb, yg, yr), (cbb, cbg, cbr), (crb, crg, crr))
MATRICES = {
    "bt601": (16, (3208, 16520, 8414), (14392, -9535, -4857), (-2341, -12051, 14392)),
    "bt709": (16, (2032, 20127, 5983), (14392, -11094, -3298), (-1320, -13072, 14392)),
    "bt601_full": (0, (3735, 19235, 9798), (16384, -10855, -5529), (-2664, -13720, 16384)),
    "bt709_full": (0, (2366, 23436, 6966), (16384, -12630, -3754), (-1502, -14882, 16384)),
}
NAMES = tuple(MATRICES)


def planes(E, matrix="bt601"):
    """(Y [H, W], Cb [H / 2, W / 2], Cr [H / 2, W / 2]) uint8 of the 8-bit B, G, R image E [H, W, 3] with even H and W."""
    E = np.asarray(E)
    assert E.ndim == 3 and E.shape[2] == 3 and E.dtype == np.uint8 and E.shape[0] % 2 == 0 and E.shape[1] % 2 == 0, E.shape
    yoff, yw, cbw, crw = MATRICES[matrix]
    e = E.astype(np.int64)
    y = (yw[0] * e[..., 0] + yw[1] * e[..., 1] + yw[2] * e[..., 2] + (yoff << 15) + 16384) >> 15
    s = e[0::2, 0::2] + e[0::2, 1::2] + e[1::2, 0::2] + e[1::2, 1::2]
    cb = np.minimum(255, (cbw[0] * s[..., 0] + cbw[1] * s[..., 1] + cbw[2] * s[..., 2] + (128 << 17) + 65536) >> 17)
    cr = np.minimum(255, (crw[0] * s[..., 0] + crw[1] * s[..., 1] + crw[2] * s[..., 2] + (128 << 17) + 65536) >> 17)
    assert y.min() >= 0 and y.max() <= 255 and cb.min() >= 0 and cr.min() >= 0
    return y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


def convert(E, fmt, matrix="bt601"):
    """The delivered tightly packed frame [3 H / 2, W] uint8."""
    assert fmt in FORMATS, fmt
    y, cb, cr = planes(E, matrix)
    h, w = y.shape
    out = np.empty((h // 2 * 3, w), np.uint8)
    out[:h] = y
    if fmt == "nv12":
        out[h:, 0::2] = cb
        out[h:, 1::2] = cr
    else:
        out[h:] = np.concatenate([cb.reshape(-1), cr.reshape(-1)]).reshape(h // 2, w)
    return out


def pitched(E, fmt, matrix, pitch, fill=0xA5, base=0, total=None):
    """One frame as the kernel lays it out at row pitch `pitch` from byte `base` of a block of `total` bytes (default: the frame's
    3 H / 2 pitches) that holds `fill` everywhere else."""
    y, cb, cr = planes(E, matrix)
    h, w = y.shape
    buf = np.full(base + pitch * (h // 2 * 3) if total is None else total, fill, np.uint8)
    for r in range(h):
        buf[base + r * pitch:base + r * pitch + w] = y[r]
    for j in range(h // 2):
        if fmt == "nv12":
            at = base + (h + j) * pitch
            buf[at:at + w:2] = cb[j]
            buf[at + 1:at + w:2] = cr[j]
        else:
            assert pitch % 2 == 0
            at = base + h * pitch + j * (pitch // 2)
            buf[at:at + w // 2] = cb[j]
            at += (h // 2) * (pitch // 2)
            buf[at:at + w // 2] = cr[j]
    return buf
