"""CLAHE of a one-channel uint8 picture in numpy, written from PARITY.md "Local contrast: CLAHE" (OpenCV 4's CLAHE_Impl::apply for
CV_8UC1, restated): the reference of tests/test_clahe.py, tests/test_clahe_gpu.py and the kernels run on the host.  Every float32
product and sum is rounded on its own; nothing here looks at the library."""
import numpy as np

F = np.float32
MAX_TILES = 16


def geometry(h, w, tiles_x, tiles_y, clip_limit):
    """(E rows, E cols, tw, th, cl, scale) of an h x w picture: steps 1 and 2."""
    eh, ew = h, w
    if w % tiles_x or h % tiles_y:
        ew, eh = w + tiles_x - w % tiles_x, h + tiles_y - h % tiles_y
    tw, th = ew // tiles_x, eh // tiles_y
    area = tw * th
    cl = max(int(min(float(clip_limit) * area / 256, float(area))), 1) if clip_limit > 0 else 0
    return eh, ew, tw, th, cl, F(255.0) / F(area)


def extend(pic, eh, ew):
    """E: reflect-101 on the right and at the bottom."""
    h, w = pic.shape
    ys = np.array([y if y < h else 2 * h - 2 - y for y in range(eh)])
    xs = np.array([x if x < w else 2 * w - 2 - x for x in range(ew)])
    return pic[np.ix_(ys, xs)]


def tile_lut(tile, cl, scale):
    """Step 3 for one tile: the 256 bytes of its table."""
    hist = np.bincount(tile.ravel(), minlength=256).astype(np.int64)
    if cl > 0:
        excess = int(np.maximum(hist - cl, 0).sum())
        hist = np.minimum(hist, cl)
        batch = excess // 256
        residual = excess - 256 * batch
        hist = hist + batch
        if residual > 0:
            step = max(256 // residual, 1)
            k = np.arange(256)
            hist = hist + ((k % step == 0) & (k // step < residual))
    s = np.cumsum(hist).astype(F)          # (float)s_k, rounded to nearest even
    return np.clip(np.rint(s * scale), 0, 255).astype(np.uint8)


def luts(pic, clip_limit, tiles_x, tiles_y):
    """uint8 [tiles_y, tiles_x, 256]."""
    h, w = pic.shape
    eh, ew, tw, th, cl, scale = geometry(h, w, tiles_x, tiles_y, clip_limit)
    e = extend(pic, eh, ew)
    out = np.empty((tiles_y, tiles_x, 256), np.uint8)
    for j in range(tiles_y):
        for i in range(tiles_x):
            out[j, i] = tile_lut(e[j * th:(j + 1) * th, i * tw:(i + 1) * tw], cl, scale)
    return out


def _axis(n, inv, tiles):
    f = np.arange(n).astype(F) * inv - F(0.5)
    c1 = np.floor(f).astype(np.int64)
    a = (f - c1.astype(F)).astype(F)
    a1 = (F(1.0) - a).astype(F)
    return np.maximum(c1, 0), np.minimum(c1 + 1, tiles - 1), a, a1


def clahe(pic, clip_limit, tiles_x, tiles_y):
    """The equalised picture: step 4 on top of luts()."""
    pic = np.ascontiguousarray(pic)
    assert pic.dtype == np.uint8 and pic.ndim == 2
    h, w = pic.shape
    assert 1 <= tiles_x <= MAX_TILES and 1 <= tiles_y <= MAX_TILES and w >= 2 * tiles_x and h >= 2 * tiles_y
    _, _, tw, th, _, _ = geometry(h, w, tiles_x, tiles_y, clip_limit)
    lut = luts(pic, clip_limit, tiles_x, tiles_y).astype(F)
    x1, x2, xa, xa1 = _axis(w, F(1.0) / F(tw), tiles_x)
    y1, y2, ya, ya1 = _axis(h, F(1.0) / F(th), tiles_y)
    v = pic.astype(np.int64)
    y1, y2, ya, ya1 = y1[:, None], y2[:, None], ya[:, None], ya1[:, None]
    x1, x2, xa, xa1 = x1[None, :], x2[None, :], xa[None, :], xa1[None, :]
    top = (lut[y1, x1, v] * xa1).astype(F) + (lut[y1, x2, v] * xa).astype(F)
    bottom = (lut[y2, x1, v] * xa1).astype(F) + (lut[y2, x2, v] * xa).astype(F)
    res = (top.astype(F) * ya1).astype(F) + (bottom.astype(F) * ya).astype(F)
    return np.clip(np.rint(res.astype(F)), 0, 255).astype(np.uint8)


def apply_to_delivered(img, rect, clip_limit, tiles_x, tiles_y):
    """A delivered one-channel image with CLAHE on its picture rectangle rect = (x, y, w, h); the bands stay."""
    x, y, w, h = rect
    out = np.array(img, copy=True)
    out[y:y + h, x:x + w] = clahe(img[y:y + h, x:x + w], clip_limit, tiles_x, tiles_y)
    return out
