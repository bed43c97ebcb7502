"""CPU reference of the 16-bit range (rip_set_debayer_16bit_range; PARITY.md "16-bit Bayer frames through the whole chain").

A bayer_*16 frame is demosaiced at 16 bits, every channel value is narrowed to 8 bits in integers, and from there on the frame
is processed exactly like a bgr8 frame holding the narrowed image -- so the expectation is the CPU oracle run on that image.
Narrowing is per pixel, so it commutes with the flip the oracle then applies."""
import numpy as np

from helpers import oracle_run
from mht_reference import mht_reference


def narrow16(img_u16, black, white):
    """n(v) = min(255, floor((510 * max(v - black, 0) + R) / (2 * R))), R = white - black, in int64: 255 (v - black) / R rounded
    half up, clamped to [0, 255]."""
    assert 0 <= black < white <= 65535, (black, white)
    v = np.asarray(img_u16).astype(np.int64)
    r = white - black
    return np.minimum(255, (510 * np.maximum(v - black, 0) + r) // (2 * r)).astype(np.uint8)


def demosaic16(O, frame, pattern, method):
    """The 16-bit BGR image D16 of a uint16 Bayer frame; pattern: 'bayer_rggb16', 'bayer_rggb8' or the bare name."""
    name = pattern.replace("bayer_", "").replace("16", "").replace("8", "")
    frame = np.ascontiguousarray(frame, np.uint16)
    if method == "mht":
        return mht_reference(frame, name)
    assert method == "bilinear", method
    return O.debayer16(frame, "bayer_%s16" % name)


def expected_raw16(O, c, frame, pattern, method, black, white, ccc=None, taps=False):
    """What oracle_run returns -- (out, encoding[, debayered tap, colour tap]) -- for a bayer_*16 frame under configuration c."""
    return oracle_run(O, c, narrow16(demosaic16(O, frame, pattern, method), black, white), "bgr8", ccc=ccc, taps=taps)
