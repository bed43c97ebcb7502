"""The resize stage under the "area" interpolation (include/rip.h rip_set_output_interpolation) restated in numpy, from PARITY.md
"Resize: area interpolation" alone: Python doubles for the tables, float32 arrays for the sums.

``axis_taps(s, d)``: the tap list of one axis -- per output a list of (source index, float32 weight).
``tables(R, C, H, W)``: both axes as the host hook returns them (first, count, packed weights) plus the whole-factor flag and scale.
``resize(F, H, W)``: F uint8 [R, C] or [R, C, 3] -> [H, W(, 3)] uint8; ``resize_stack`` for [n, ...].
``box_mean(F, H, W)``: the exact float64 area mean, the independent yardstick (not bit-comparable).

Everything but ``box_mean`` is compared at tolerance 0."""
import math

import numpy as np

MAX_FACTOR = 256


def check_sizes(R, C, H, W):
    assert all(1 <= v <= 16384 for v in (R, C, H, W)), (R, C, H, W)
    assert H <= R and W <= C, "area is a downscale filter"
    assert R <= MAX_FACTOR * H and C <= MAX_FACTOR * W, "factors up to 256"


def axis_taps(s, d):
    scale = float(s) / float(d)
    out = []
    for i in range(d):
        f1 = i * scale
        f2 = f1 + scale
        cell = min(scale, s - f1)
        s1 = math.ceil(f1)
        s2 = min(math.floor(f2), s - 1)
        s1 = min(s1, s2)
        taps = []
        if s1 - f1 > 1e-3:
            taps.append((s1 - 1, np.float32((s1 - f1) / cell)))
        for k in range(s1, s2):
            taps.append((k, np.float32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            taps.append((s2, np.float32(min(min(f2 - s2, 1.0), cell) / cell)))
        out.append(taps)
    return out


def is_whole(R, C, H, W):
    return R % H == 0 and C % W == 0 and (R, C) != (H, W) and (R, C) != (2 * H, 2 * W)


def tables(R, C, H, W):
    check_sizes(R, C, H, W)
    t = {}
    for name, (s, d) in (("x", (C, W)), ("y", (R, H))):
        taps = axis_taps(s, d)
        t[name + "first"] = np.array([tp[0][0] for tp in taps], np.int32)
        t[name + "count"] = np.array([len(tp) for tp in taps], np.int32)
        t[name + "weight"] = np.array([w for tp in taps for _, w in tp], np.float32)
        t[name + "index"] = [[k for k, _ in tp] for tp in taps]
    whole = is_whole(R, C, H, W)
    t["whole"] = int(whole)
    t["scale"] = np.float32(1.0) / np.float32((R // H) * (C // W)) if whole else np.float32(0)
    return t


def _padded(taps, limit):
    """index [d, n] and float32 weight [d, n] of an axis, short lists padded with weight-0 taps of an in-range index: they add +0.0"""
    n = max(len(tp) for tp in taps)
    idx = np.zeros((len(taps), n), np.int64)
    wgt = np.zeros((len(taps), n), np.float32)
    for i, tp in enumerate(taps):
        for j, (k, w) in enumerate(tp):
            idx[i, j], wgt[i, j] = k, w
        idx[i, len(tp):] = tp[-1][0]
    assert idx.min() >= 0 and idx.max() < limit
    return idx, wgt


def _to_byte(acc):
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def resize(image, H, W):
    f = np.asarray(image)
    assert f.dtype == np.uint8 and f.ndim in (2, 3), (f.dtype, f.shape)
    R, C = f.shape[:2]
    check_sizes(R, C, H, W)
    if (R, C) == (H, W):
        return f.copy()
    s = f.reshape(R, C, -1)
    cn = s.shape[2]
    if (R, C) == (2 * H, 2 * W):
        i = s.astype(np.int64)
        return ((i[0::2, 0::2] + i[0::2, 1::2] + i[1::2, 0::2] + i[1::2, 1::2] + 2) >> 2).astype(np.uint8).reshape((H, W) + f.shape[2:])
    if is_whole(R, C, H, W):
        ky, kx = R // H, C // W
        total = s.astype(np.int64).reshape(H, ky, W, kx, cn).sum(axis=(1, 3))
        assert total.max() < 1 << 24
        scale = np.float32(1.0) / np.float32(ky * kx)
        return _to_byte(total.astype(np.float32) * scale).reshape((H, W) + f.shape[2:])
    xi, xw = _padded(axis_taps(C, W), C)
    yi, yw = _padded(axis_taps(R, H), R)
    sf = s.astype(np.float32)
    # buf[r, x] of every source row r: ((0 + S[r][sx_0] a_0) + S[r][sx_1] a_1) + ..., every product and every sum rounded to float32
    buf = np.zeros((R, W, cn), np.float32)
    for k in range(xi.shape[1]):
        prod = sf[:, xi[:, k], :] * xw[None, :, k, None]
        buf = buf + prod
    assert buf.dtype == np.float32
    acc = yw[:, 0, None, None] * buf[yi[:, 0]]
    for j in range(1, yi.shape[1]):
        prod = yw[:, j, None, None] * buf[yi[:, j]]
        acc = acc + prod
    assert acc.dtype == np.float32
    return _to_byte(acc).reshape((H, W) + f.shape[2:])


def resize_stack(images, H, W):
    return np.stack([resize(f, H, W) for f in images])


def box_mean(image, H, W):
    """The mean of F over the source rectangle of every output pixel, in float64 with exact overlap lengths."""
    f = np.asarray(image).astype(np.float64)
    R, C = f.shape[:2]

    def overlap(s, d):
        m = np.zeros((d, s))
        scale = s / d
        for i in range(d):
            lo, hi = i * scale, (i + 1) * scale
            for k in range(int(math.floor(lo)), min(int(math.ceil(hi)), s)):
                m[i, k] = max(0.0, min(hi, k + 1) - max(lo, k))
            m[i] /= m[i].sum()
        return m

    my, mx = overlap(R, H), overlap(C, W)
    out = np.tensordot(my, f, axes=(1, 0))            # [H, C, ...]
    return np.moveaxis(np.tensordot(mx, out, axes=(1, 1)), 0, 1)   # [H, W, ...]
