"""The resize stage under "linear_aa" and "cubic_aa" in numpy, written from PARITY.md "Resize: antialiased filters": what
torch.nn.functional.interpolate(uint8, mode='bilinear' | 'bicubic', antialias=True, align_corners=False) computes.  Tables in Python
floats (double), one statement per step of the definition; the passes in int32.  tests/test_resize_aa.py pins this file to torch
itself, byte for byte; the host tables and the kernels are compared with this file.

Importable without a GPU and without the library."""
import functools

import numpy as np

MAX_FACTOR = 64
TILE_W = 64
LDS_BYTES = 65536


def k_linear(t):
    t = abs(t)
    return 1.0 - t if t < 1.0 else 0.0


def k_cubic(t):
    a = -0.5
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    if t < 2.0:
        return (((t - 5.0) * t + 8.0) * t - 4.0) * a
    return 0.0


FILTERS = {"linear_aa": (k_linear, 1), "cubic_aa": (k_cubic, 2)}
TORCH_MODE = {"linear_aa": "bilinear", "cubic_aa": "bicubic"}


@functools.lru_cache(maxsize=None)
def axis(name, s, d):
    """The tap lists of one axis from s to d samples: dict of first, count, wofs (int32 [d]), weight (int16, packed in output order),
    prec, and w (the normalised double weights, packed alike)."""
    k, S = FILTERS[name]
    scale = s / d
    support = S * scale if scale >= 1.0 else float(S)
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    first, count, w = [], [], []
    for i in range(d):
        c = scale * (i + 0.5)
        lo = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), s) - lo
        taps = [k((j + lo - c + 0.5) * inv) for j in range(n)]
        t = 0.0
        for v in taps:
            t += v
        if t != 0:
            taps = [v / t for v in taps]
        first.append(lo)
        count.append(n)
        w.extend(taps)
    wmax = max(w)
    prec = 0
    while prec < 22 and int(0.5 + wmax * (1 << (prec + 1))) < (1 << 15):
        prec += 1
    q = [int(0.5 + v * (1 << prec)) if v >= 0 else int(-0.5 + v * (1 << prec)) for v in w]
    assert all(-32768 <= v <= 32767 for v in q)
    count_a = np.array(count, np.int32)
    out = dict(first=np.array(first, np.int32), count=count_a, wofs=(np.cumsum(count_a) - count_a).astype(np.int32), weight=np.array(q, np.int16),
               prec=prec, w=np.array(w, np.float64))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def one_pass(img, t, unclipped=None):
    """img: uint8 [n, s, ...] filtered along axis 1 by the tables t; unclipped (a list) receives (min, max) of the values before the clamp."""
    d = len(t["first"])
    out = np.empty((img.shape[0], d) + img.shape[2:], np.uint8)
    lo, hi = 0, 255
    for i in range(d):
        f, n, o = int(t["first"][i]), int(t["count"][i]), int(t["wofs"][i])
        q = t["weight"][o:o + n].astype(np.int32).reshape((1, n) + (1,) * (img.ndim - 2))
        acc = (img[:, f:f + n].astype(np.int32) * q).sum(axis=1, dtype=np.int32) + (1 << (t["prec"] - 1))
        v = acc >> t["prec"]
        lo, hi = min(lo, int(v.min())), max(hi, int(v.max()))
        out[:, i] = np.clip(v, 0, 255)
    if unclipped is not None:
        unclipped.append((lo, hi))
    return out


def resize(img, H, W, name, unclipped=None):
    """img: uint8 [R, C] or [R, C, channels] -> [H, W(, channels)]: the horizontal pass over every source row, rounded to uint8, then
    the vertical pass; a pass whose axis keeps its size is skipped."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    R, C = img.shape[:2]
    x = img.reshape(R, C, -1)
    if W != C:
        x = one_pass(x.transpose(1, 0, 2)[None], axis(name, C, W), unclipped)[0].transpose(1, 0, 2)
    if H != R:
        x = one_pass(x[None], axis(name, R, H), unclipped)[0]
    return np.ascontiguousarray(x.reshape((H, W) + img.shape[2:]))


def resize_stack(frames, H, W, name):
    return np.stack([resize(f, H, W, name) for f in frames])


def tile_rows(name, R, H, channels):
    """(tile height, LDS rows) of the kernel: the largest of 8, 4, 2, 1 whose largest span of source rows x 64 x channels fits 64 KiB."""
    t = None if R == H else axis(name, R, H)
    for th in (8, 4, 2, 1):
        span = 0
        for y0 in range(0, H, th):
            y1 = min(H, y0 + th) - 1
            span = max(span, y1 - y0 + 1 if t is None else int(t["first"][y1] + t["count"][y1] - t["first"][y0]))
        if span * TILE_W * channels <= LDS_BYTES or th == 1:
            return th, span


def torch_resize(img, H, W, name, channels_last=False):
    """The same through torch itself (CPU): img uint8 [R, C(, channels)]."""
    import torch
    import torch.nn.functional as F
    a = np.asarray(img)
    x = torch.from_numpy(np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1], -1))).permute(2, 0, 1)[None]
    x = x.contiguous(memory_format=torch.channels_last) if channels_last else x.contiguous()
    y = F.interpolate(x, size=(H, W), mode=TORCH_MODE[name], antialias=True, align_corners=False)
    return np.ascontiguousarray(y[0].permute(1, 2, 0).numpy()).reshape((H, W) + a.shape[2:])
