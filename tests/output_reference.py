"""The output stage (include/rip.h rip_set_output_format) restated in numpy, from the definition alone.

``convert(E, fmt, divisor, mean, std)``: E is the pipeline's final image, uint8 [R, C, 3] in B, G, R order (or a stack
[n, R, C, 3]); the result is what the frame calls deliver under format ``fmt``:

  rgb8            E with the channels reversed, uint8 [R, C, 3]
  mono8           (3735 B + 19235 G + 9798 R + 16384) >> 15 in integers, uint8 [R, C]
  {rgb,bgr}_chw_* planes (R, G, B) or (B, G, R) of T_c[v], [3, R, C]: y = (v / divisor - mean_c) / std_c in float64 with every
                  operation rounded, T_c[v] = float32(y); f16 = float32 -> float16 by numpy (round to nearest even), bf16 =
                  an explicit round to nearest even on the float32's bits, returned as uint16 bit patterns.

Float results are compared as bit patterns (``bits``): the tolerance is 0 everywhere."""
import numpy as np

TABLE_FORMATS = ("rgb_chw_f32", "rgb_chw_f16", "rgb_chw_bf16", "bgr_chw_f32", "bgr_chw_f16", "bgr_chw_bf16")
FORMATS = ("rgb8", "mono8") + TABLE_FORMATS
ELEM_BYTES = {"rgb8": 1, "mono8": 1, "rgb_chw_f32": 4, "rgb_chw_f16": 2, "rgb_chw_bf16": 2, "bgr_chw_f32": 4, "bgr_chw_f16": 2,
              "bgr_chw_bf16": 2}
DEFAULT_NORM = (255.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
IMAGENET_MEAN_RGB, IMAGENET_STD_RGB = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def is_planar(fmt):
    return fmt in TABLE_FORMATS


def bf16_bits(f32):
    """float32 array -> bfloat16 bit patterns (uint16), round to nearest even on the upper 16 bits; no NaN expected."""
    u = np.ascontiguousarray(f32, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def table(fmt, divisor=255.0, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
    """[3, 256] in the format's element type (bf16: uint16 bit patterns), plane-major."""
    assert fmt in TABLE_FORMATS, fmt
    v = np.arange(256, dtype=np.float64)[None, :]
    m = np.asarray(mean, np.float64)[:, None]
    s = np.asarray(std, np.float64)[:, None]
    with np.errstate(over="ignore", divide="ignore"):
        y = ((v / np.float64(divisor)) - m) / s
        t = y.astype(np.float32)
        if fmt.endswith("_f32"):
            return t
        if fmt.endswith("_bf16"):
            return bf16_bits(t)
        return t.astype(np.float16)


def mono8(bgr):
    a = np.asarray(bgr, np.uint8).astype(np.int64)
    return ((3735 * a[..., 0] + 19235 * a[..., 1] + 9798 * a[..., 2] + 16384) >> 15).astype(np.uint8)


def convert(image, fmt, divisor=255.0, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
    e = np.asarray(image)
    assert e.dtype == np.uint8 and e.shape[-1] == 3, (e.dtype, e.shape)
    if fmt == "rgb8":
        return np.ascontiguousarray(e[..., ::-1])
    if fmt == "mono8":
        return mono8(e)
    t = table(fmt, divisor, mean, std)
    order = (2, 1, 0) if fmt.startswith("rgb") else (0, 1, 2)
    planes = [t[c][e[..., ch]] for c, ch in enumerate(order)]
    return np.stack(planes, axis=-3)   # [3, R, C] or [n, 3, R, C]


def bits(a):
    """The array as unsigned integers of its element size: how float results are compared."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])
