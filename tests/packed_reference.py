"""numpy pack / unpack of the packed 10- and 12-bit Bayer layouts (include/rip.h "Packed Bayer frames"), written from the
layouts' definitions and independent of the C code.

  10p      PFNC lsb-first bit stream: sample x is bits [10 x, 10 x + 10) of the row read as a little-endian bit string
  12p      the same with 12 bits
  10_csi2  MIPI CSI-2 RAW10: four samples in five bytes -- their upper 8 bits, then one byte of the four 2-bit remainders,
           sample j of the group in bits [2 j, 2 j + 2)
  12_csi2  MIPI CSI-2 RAW12: two samples in three bytes -- their upper 8 bits, then one byte of the two 4-bit remainders, the
           even sample's in the low nibble

A packed frame is a 2-D uint8 array [rows, row bytes]; the CPU expectation of the library on it is
tests/raw16_reference.py::expected_raw16 on ``unpack`` of it."""
import numpy as np

LAYOUTS = ("10p", "12p", "10_csi2", "12_csi2")
BITS = {"10p": 10, "12p": 12, "10_csi2": 10, "12_csi2": 12}
WIDTH_MULTIPLE = {"10p": 1, "12p": 1, "10_csi2": 4, "12_csi2": 2}   # whole CSI-2 groups
GROUP = {"10p": 4, "12p": 2, "10_csi2": 4, "12_csi2": 2}            # samples after which the byte pattern repeats
NAMES = ("rggb", "bggr", "gbrg", "grbg")


def enc(name, layout):
    return "bayer_%s%s" % (name, layout)


def row_bytes(cols, layout):
    return (cols * BITS[layout] + 7) // 8


def natural_range(layout):
    return 0, (1 << BITS[layout]) - 1


def allowed_width(w, layout):
    """The nearest width >= max(w, 3) the layout allows."""
    m = WIDTH_MULTIPLE[layout]
    return (max(w, 3) + m - 1) // m * m


def pack(frame_u16, layout, fill_bits=0):
    """[rows, cols] samples below 2^B -> [rows, row bytes] uint8.  fill_bits: 0 or 1, the value of the bits of a row's last
    byte that lie beyond its last pixel (p layouts)."""
    f = np.asarray(frame_u16).astype(np.uint32)
    rows, cols = f.shape
    b = BITS[layout]
    assert int(f.max(initial=0)) < (1 << b), "sample does not fit %d bits" % b
    assert cols % WIDTH_MULTIPLE[layout] == 0, (cols, layout)
    if layout in ("10p", "12p"):
        bits = ((f[:, :, None] >> np.arange(b, dtype=np.uint32)) & 1).astype(np.uint8).reshape(rows, cols * b)
        pad = row_bytes(cols, layout) * 8 - cols * b
        bits = np.concatenate([bits, np.full((rows, pad), fill_bits, np.uint8)], axis=1)
        return np.packbits(bits, axis=1, bitorder="little")
    if layout == "10_csi2":
        g = f.reshape(rows, cols // 4, 4)
        low = (g[:, :, 0] & 3) | (g[:, :, 1] & 3) << 2 | (g[:, :, 2] & 3) << 4 | (g[:, :, 3] & 3) << 6
        return np.concatenate([g >> 2, low[:, :, None]], axis=2).astype(np.uint8).reshape(rows, cols // 4 * 5)
    assert layout == "12_csi2", layout
    g = f.reshape(rows, cols // 2, 2)
    low = (g[:, :, 0] & 15) | (g[:, :, 1] & 15) << 4
    return np.concatenate([g >> 4, low[:, :, None]], axis=2).astype(np.uint8).reshape(rows, cols // 2 * 3)


def unpack(packed, cols, layout):
    """[rows, >= row bytes] uint8 -> [rows, cols] uint16; bytes beyond a row's payload and bits beyond its last pixel are not
    interpreted."""
    p = np.asarray(packed)
    assert p.dtype == np.uint8 and p.ndim == 2
    assert cols % WIDTH_MULTIPLE[layout] == 0, (cols, layout)
    rows = p.shape[0]
    b = BITS[layout]
    p = p[:, :row_bytes(cols, layout)]
    if layout in ("10p", "12p"):
        bits = np.unpackbits(p, axis=1, bitorder="little")[:, :cols * b].reshape(rows, cols, b).astype(np.uint32)
        return (bits << np.arange(b, dtype=np.uint32)).sum(axis=2).astype(np.uint16)
    if layout == "10_csi2":
        g = p.reshape(rows, cols // 4, 5).astype(np.uint32)
        low = (g[:, :, 4:5] >> (2 * np.arange(4, dtype=np.uint32))) & 3
        return (g[:, :, :4] << 2 | low).reshape(rows, cols).astype(np.uint16)
    assert layout == "12_csi2", layout
    g = p.reshape(rows, cols // 2, 3).astype(np.uint32)
    low = (g[:, :, 2:3] >> (4 * np.arange(2, dtype=np.uint32))) & 15
    return (g[:, :, :2] << 4 | low).reshape(rows, cols).astype(np.uint16)


def pitched(packed, pitch, fill):
    """The rows of ``packed`` inside a [rows, pitch] array whose other bytes hold ``fill``: (the view of the rows, the array)."""
    rows, rb = packed.shape
    assert pitch >= rb
    wide = np.full((rows, pitch), fill, np.uint8)
    wide[:, :rb] = packed
    return wide[:, :rb], wide


def lib_unpack(lib, encoding, packed, cols, step=None):
    """rip_debug_unpack; returns (status, [rows, cols] uint16)."""
    import ctypes as C
    p = np.asarray(packed)
    assert p.dtype == np.uint8 and p.ndim == 2 and p.strides[1] == 1
    out = np.full((p.shape[0], cols), 0xFFFF, np.uint16)
    lib.rip_debug_unpack.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    st = lib.rip_debug_unpack(encoding.encode(), p.ctypes.data_as(C.c_void_p), C.c_size_t(p.strides[0] if step is None else step),
                              p.shape[0], cols, out.ctypes.data_as(C.c_void_p))
    return st, out
