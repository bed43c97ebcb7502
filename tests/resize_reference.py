"""The resize stage (include/rip.h rip_set_output_size) restated in numpy, from PARITY.md "Resize" alone.

``tables(R, C, H, W)``: the per-axis tables -- xofs [W], alpha [W, 2], yofs [H, 2] (the two clamped rows), beta [H, 2], area2.
``resize(F, H, W)``: F uint8 [R, C] or [R, C, 3] (or a stack [n, ...] with ``resize_stack``) -> [H, W(, 3)], in int64.
``scaled_camera(K, P, R, C, H, W)``: the camera matrices of the delivered image, in Python floats.

Everything is compared at tolerance 0."""
import numpy as np


def _axis(src, dst, reset):
    """(first tap, f) of every output position of one axis: float32 where PARITY.md says float."""
    x = np.arange(dst, dtype=np.float64)
    f = ((x + 0.5) * (np.float64(src) / np.float64(dst)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if reset:
        low, high = s < 0, s >= src - 1
        f = np.where(low | high, np.float32(0), f).astype(np.float32)
        s = np.where(low, 0, np.where(high, src - 1, s))
    return s, f


def _weights(f):
    """cvRound((1.f - f) * 2048), cvRound(f * 2048): float32 products, rounded half to even (np.rint)."""
    one = np.float32(1)
    w0 = np.rint(((one - f).astype(np.float32) * np.float32(2048)).astype(np.float32)).astype(np.int64)
    w1 = np.rint((f * np.float32(2048)).astype(np.float32)).astype(np.int64)
    return np.stack([w0, w1], axis=1)


def tables(R, C, H, W):
    sx, fx = _axis(C, W, reset=True)
    sy, fy = _axis(R, H, reset=False)
    yofs = np.stack([np.clip(sy, 0, R - 1), np.clip(sy + 1, 0, R - 1)], axis=1)
    return dict(xofs=sx, alpha=_weights(fx), yofs=yofs, beta=_weights(fy), area2=int(R == 2 * H and C == 2 * W))


def resize(image, H, W):
    f = np.asarray(image)
    assert f.dtype == np.uint8 and f.ndim in (2, 3), (f.dtype, f.shape)
    R, C = f.shape[:2]
    s = f.astype(np.int64)
    if R == 2 * H and C == 2 * W:
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    t = tables(R, C, H, W)
    sx, sx1 = t["xofs"], np.minimum(t["xofs"] + 1, C - 1)
    a = t["alpha"].reshape((W, 2) + (1,) * (f.ndim - 2))
    b = t["beta"].reshape((H, 2) + (1,) * (f.ndim - 1))
    h0 = s[t["yofs"][:, 0]][:, sx] * a[:, 0] + s[t["yofs"][:, 0]][:, sx1] * a[:, 1]
    h1 = s[t["yofs"][:, 1]][:, sx] * a[:, 0] + s[t["yofs"][:, 1]][:, sx1] * a[:, 1]
    out = (((b[:, 0] * (h0 >> 4)) >> 16) + ((b[:, 1] * (h1 >> 4)) >> 16) + 2) >> 2
    return (out & 255).astype(np.uint8)


def resize_stack(images, H, W):
    return np.stack([resize(f, H, W) for f in images])


def scaled_camera(K, P, R, C, H, W):
    """K [3, 3], P [3, 4] of an R x C image -> those of its H x W resize (pixel centres at half-integers)."""
    k = [float(v) for v in np.asarray(K, np.float64).reshape(-1)]
    p = [float(v) for v in np.asarray(P, np.float64).reshape(-1)]
    if (R, C) != (H, W):
        a, b = float(W) / float(C), float(H) / float(R)
        k[0] *= a
        k[1] *= a
        k[2] = a * (k[2] + 0.5) - 0.5
        k[4] *= b
        k[5] = b * (k[5] + 0.5) - 0.5
        p[0] *= a
        p[1] *= a
        p[2] = a * (p[2] + 0.5) - 0.5
        p[3] *= a
        p[5] *= b
        p[6] = b * (p[6] + 0.5) - 0.5
        p[7] *= b
    return np.array(k, np.float64).reshape(3, 3), np.array(p, np.float64).reshape(3, 4)
