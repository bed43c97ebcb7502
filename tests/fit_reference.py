"""The window and the fit modes of the resize stage (include/rip.h rip_set_output_roi, rip_set_output_fit, rip_set_output_pad)
restated in numpy, from PARITY.md "Resize: window and fit" alone.

``geometry(C, R, roi, target, fit)``: (src_xywh, dst_xywh, (W, H) delivered) -- Python integers, C division (all operands >= 0).
``expected(F, roi, target, fit, interpolation, pad)``: the delivered image of F uint8 [R, C] or [R, C, 3]: a canvas of pad bytes with
the picture pasted in; the picture is tests/resize_reference.py or tests/area_reference.py applied to the cropped window.
``camera(K, P, C, R, roi, target, fit)``: (height, width, K, P) of the delivered image in Python floats.

Everything is compared at tolerance 0."""
import numpy as np

import area_reference as A
import resize_reference as Z

FITS = ("stretch", "letterbox", "crop")
PAD_DEFAULT = (114, 114, 114)


class Outside(ValueError):
    """the window does not lie inside F"""


def clamp(v, lo, hi):
    return min(max(v, lo), hi)


def geometry(C, R, roi=None, target=None, fit="stretch"):
    assert fit in FITS
    x, y, w, h = (0, 0, C, R) if roi is None or tuple(roi) == (0, 0, 0, 0) else roi
    if x + w > C or y + h > R:
        raise Outside((x, y, w, h, C, R))
    if target is None or tuple(target) == (0, 0):
        return (x, y, w, h), (0, 0, w, h), (w, h)
    W, H = target
    left, top, wi, hi = 0, 0, W, H
    if fit == "crop":
        if w * H >= h * W:
            w2 = clamp((2 * h * W + H) // (2 * H), 1, w)
            x, w = x + (w - w2) // 2, w2
        else:
            h2 = clamp((2 * w * H + W) // (2 * W), 1, h)
            y, h = y + (h - h2) // 2, h2
    elif fit == "letterbox":
        if W * h <= H * w:
            hi = clamp((2 * h * W + w) // (2 * w), 1, H)
        else:
            wi = clamp((2 * w * H + h) // (2 * h), 1, W)
        left, top = (W - wi) // 2, (H - hi) // 2
    return (x, y, w, h), (left, top, wi, hi), (W, H)


def pad_bytes(pad, channels):
    b, g, r = pad
    return (b, g, r) if channels == 3 else ((3735 * b + 19235 * g + 9798 * r + 16384) >> 15,)


def picture(window, hi, wi, interpolation):
    """The existing stage on a frame that holds only the window: the copy, the 2 x 2 mean and the linear tables are
    resize_reference's, whole factors and tap lists area_reference's."""
    h, w = window.shape[:2]
    if interpolation == "area" and (h, w) != (hi, wi):
        return A.resize(window, hi, wi)
    return Z.resize(window, hi, wi)


def expected(F, roi=None, target=None, fit="stretch", interpolation="linear", pad=PAD_DEFAULT):
    F = np.asarray(F)
    R, C = F.shape[:2]
    (x, y, w, h), (left, top, wi, hi), (W, H) = geometry(C, R, roi, target, fit)
    channels = 1 if F.ndim == 2 else 3
    canvas = np.empty((H, W) + F.shape[2:], np.uint8)
    canvas[...] = np.array(pad_bytes(pad, channels), np.uint8) if channels == 3 else pad_bytes(pad, 1)[0]
    canvas[top:top + hi, left:left + wi] = picture(np.ascontiguousarray(F[y:y + h, x:x + w]), hi, wi, interpolation)
    return canvas


def expected_stack(frames, *args, **kw):
    return np.stack([expected(f, *args, **kw) for f in frames])


def camera(K, P, C, R, roi=None, target=None, fit="stretch"):
    (xs, ys, ws, hs), (left, top, wi, hi), (W, H) = geometry(C, R, roi, target, fit)
    k = [float(v) for v in np.asarray(K, np.float64).reshape(-1)]
    p = [float(v) for v in np.asarray(P, np.float64).reshape(-1)]
    a, b = float(wi) / float(ws), float(hi) / float(hs)
    xs, ys, left, top = float(xs), float(ys), float(left), float(top)
    k[0] *= a
    k[1] *= a
    k[2] = (a * ((k[2] - xs) + 0.5) - 0.5) + left
    k[4] *= b
    k[5] = (b * ((k[5] - ys) + 0.5) - 0.5) + top
    p[0] *= a
    p[1] *= a
    p[2] = (a * ((p[2] - xs) + 0.5) - 0.5) + left
    p[3] *= a
    p[5] *= b
    p[6] = (b * ((p[6] - ys) + 0.5) - 0.5) + top
    p[7] *= b
    return H, W, np.array(k, np.float64).reshape(3, 3), np.array(p, np.float64).reshape(3, 4)


def rule(window_wh, picture_wh, interpolation):
    """Which resize rule applies to (window size -> picture size): "copy" and "linear" are the linear tables, "mean2" the 2 x 2
    mean, "whole" and "taps" the area interpolation's."""
    (w, h), (wi, hi) = window_wh, picture_wh
    if (w, h) == (wi, hi):
        return "copy"
    if (w, h) == (2 * wi, 2 * hi):
        return "mean2"
    if interpolation == "area":
        return "whole" if w % wi == 0 and h % hi == 0 else "taps"
    return "linear"


def kernel_name(channels, kind, windowed):
    """The kernel a rule runs: librip_fit_hip.so's when a window other than all of F is read, the existing libraries' otherwise."""
    if windowed:
        return {"copy": "fit_linear_kernel<%d>", "linear": "fit_linear_kernel<%d>", "mean2": "fit_mean2_kernel<%d>",
                "whole": "fit_area_kernel<%d, true>", "taps": "fit_area_kernel<%d, false>"}[kind] % channels
    return {"copy": "resize_kernel<%d, false>", "linear": "resize_kernel<%d, false>", "mean2": "resize_kernel<%d, true>",
            "whole": "area_reduce_kernel<%d, true>", "taps": "area_reduce_kernel<%d, false>"}[kind] % channels
