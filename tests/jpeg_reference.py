"""The JPEG output format (include/rip.h rip_set_output_jpeg; PARITY.md "Output formats: JPEG") restated in numpy int64 and plain
Python, from the definition and not from the kernels: extension to whole MCUs, the bt601_full planes of tests/yuv_reference.py, the
integer forward DCT, the IJG-scaled Annex K tables, ties-away quantisation, the Annex K Huffman tables, restart intervals, the header.

``encode`` writes a stream; ``decode_coefficients`` is a small baseline parser and Huffman decoder that shares no code with the
writer (it builds its code tables from the DHT segments of the stream it reads).  Importable without a GPU."""
import numpy as np

import yuv_reference as YR

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4"
    "c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))
HEADER_BYTES = {1: 330, 3: 613}
# the forward DCT's constants: round(c * 2^13)
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def quant_tables(quality):
    """(luminance, chrominance) divisors Q in natural (row-major) order for a quality in 1..100."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA))


def extend(picture, mcu):
    """The picture with its last column and row repeated up to multiples of the MCU."""
    h, w = picture.shape[:2]
    pad = [(0, -h % mcu), (0, -w % mcu)] + [(0, 0)] * (picture.ndim - 2)
    return np.pad(picture, pad, mode="edge")


def planes(picture):
    """The component planes of the extended picture: [Y] of a one-channel picture, [Y, Cb, Cr] (bt601_full, 4:2:0) of B, G, R."""
    picture = np.asarray(picture)
    assert picture.dtype == np.uint8
    if picture.ndim == 2:
        return [extend(picture, 8)]
    return list(YR.planes(extend(picture, 16), "bt601_full"))


def _pass(d, first):
    """One pass of the transform over the last axis of int64 d [..., 8]."""
    rnd = lambda x, n: (x + (1 << (n - 1))) >> n
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    n = 11 if first else 15
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[..., 0], out[..., 4] = rnd(t10 + t11, 2), rnd(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541
    out[..., 2] = rnd(z1 + t13 * F_0_765, n)
    out[..., 6] = rnd(z1 - t12 * F_1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    out[..., 7] = rnd(t4 + z1 + z3, n)
    out[..., 5] = rnd(t5 + z2 + z4, n)
    out[..., 3] = rnd(t6 + z2 + z3, n)
    out[..., 1] = rnd(t7 + z1 + z4, n)
    return out


def fdct(blocks):
    """Eight times the DCT coefficients (JPEG normalisation) of uint8 blocks [..., 8, 8], level shift 128: rows first, then columns."""
    d = np.asarray(blocks).astype(np.int64) - 128
    d = _pass(d, True)
    return np.swapaxes(_pass(np.swapaxes(d, -1, -2).copy(), False), -1, -2)


def quantise(coef8, q):
    """Round to nearest, ties away from zero, of coef8 / (8 q); clamped to +-1023."""
    d = 8 * np.asarray(q).astype(np.int64).reshape(8, 8)
    a = (np.abs(coef8) + d // 2) // d
    return np.sign(coef8) * np.minimum(a, 1023)


def reciprocal(q):
    """The kernel's constant for a divisor Q: ceil(2^32 / (8 Q)); (a * r) >> 32 == a // (8 Q) for a < 2^16."""
    return -(-(1 << 32) // (8 * int(q)))


def plane_blocks(plane, q):
    """Quantised coefficients [by, bx, 64] in zigzag order of one plane."""
    h, w = plane.shape
    b = plane.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)
    return quantise(fdct(b), q).reshape(h // 8, w // 8, 64)[..., ZIGZAG]


def scan_blocks(picture, quality):
    """[(component, coefficients [64] in zigzag order)] in scan order, and MCUs per row / MCU rows."""
    ps = planes(picture)
    ql, qc = quant_tables(quality)
    if len(ps) == 1:
        b = plane_blocks(ps[0], ql)
        return [(0, b[y, x]) for y in range(b.shape[0]) for x in range(b.shape[1])], b.shape[1], b.shape[0]
    by, bcb, bcr = plane_blocks(ps[0], ql), plane_blocks(ps[1], qc), plane_blocks(ps[2], qc)
    out = []
    for y in range(bcb.shape[0]):
        for x in range(bcb.shape[1]):
            out += [(0, by[2 * y + i, 2 * x + j]) for i in (0, 1) for j in (0, 1)] + [(1, bcb[y, x]), (2, bcr[y, x])]
    return out, bcb.shape[1], bcb.shape[0]


def component_blocks(picture, quality):
    """Per component the quantised blocks [n, 64] in the order the scan visits them."""
    blocks, _, _ = scan_blocks(picture, quality)
    ncomp = 1 if np.asarray(picture).ndim == 2 else 3
    return [np.array([b for c, b in blocks if c == k]) for k in range(ncomp)]


def _codes(bits, vals):
    """{symbol: bit string} of a table given as Annex C builds it."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = format(code, "0%db" % length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def _magnitude(v):
    v = int(v)
    size = abs(v).bit_length()
    return size, (format(v if v > 0 else v + (1 << size) - 1, "0%db" % size) if size else "")


def _block_bits(coef, pred, dc, ac):
    size, extra = _magnitude(int(coef[0]) - pred)
    out = [dc[size], extra]
    run = 0
    last = max([k for k in range(1, 64) if coef[k]], default=0)
    for k in range(1, last + 1):
        if coef[k] == 0:
            run += 1
            continue
        while run > 15:
            out.append(ac[0xF0])
            run -= 16
        size, extra = _magnitude(coef[k])
        out += [ac[(run << 4) | size], extra]
        run = 0
    if last < 63:
        out.append(ac[0x00])
    return "".join(out)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(h, w, ncomp, quality, restart_rows):
    ql, qc = quant_tables(quality)
    mcu = 8 if ncomp == 1 else 16
    out = bytes([0xFF, 0xD8]) + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    dqt = bytes([0]) + bytes(int(v) for v in ql[ZIGZAG])
    dht = bytes([0x00] + DC_LUMA[0] + DC_LUMA[1]) + bytes([0x10] + AC_LUMA[0] + AC_LUMA[1])
    if ncomp == 3:
        dqt += bytes([1]) + bytes(int(v) for v in qc[ZIGZAG])
        dht += bytes([0x01] + DC_CHROMA[0] + DC_CHROMA[1]) + bytes([0x11] + AC_CHROMA[0] + AC_CHROMA[1])
    out += _segment(0xDB, dqt)
    comps = [(1, 0x11 if ncomp == 1 else 0x22, 0)] + ([(2, 0x11, 1), (3, 0x11, 1)] if ncomp == 3 else [])
    out += _segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([ncomp]) + bytes(v for c in comps for v in c))
    out += _segment(0xC4, dht)
    out += _segment(0xDD, (restart_rows * (-(-w // mcu))).to_bytes(2, "big"))
    out += _segment(0xDA, bytes([ncomp]) + bytes(v for c in comps for v in (c[0], 0x00 if c[2] == 0 else 0x11)) + bytes([0, 63, 0]))
    assert len(out) == HEADER_BYTES[ncomp]
    return out


def default_slot(h, w, ncomp, restart_rows):
    mcu = 8 if ncomp == 1 else 16
    eh, ew = h + -h % mcu, w + -w % mcu
    intervals = -(-(eh // mcu) // restart_rows)
    return HEADER_BYTES[ncomp] + (eh * ew * 3 // 2 if ncomp == 3 else eh * ew) + 2 * intervals + 2


def encode(picture, quality=90, restart_rows=1):
    """The stream of a uint8 picture [H, W] or [H, W, 3] (B, G, R)."""
    picture = np.asarray(picture)
    h, w = picture.shape[:2]
    ncomp = 1 if picture.ndim == 2 else 3
    blocks, mcux, mcuy = scan_blocks(picture, quality)
    per_mcu = 1 if ncomp == 1 else 6
    tables = [(_codes(*DC_LUMA), _codes(*AC_LUMA))] + [(_codes(*DC_CHROMA), _codes(*AC_CHROMA))] * 2
    out = bytearray(header(h, w, ncomp, quality, restart_rows))
    intervals = -(-mcuy // restart_rows)
    for iv in range(intervals):
        first, end = iv * restart_rows * mcux * per_mcu, min((iv + 1) * restart_rows, mcuy) * mcux * per_mcu
        pred, bits = [0, 0, 0], []
        for c, coef in blocks[first:end]:
            bits.append(_block_bits(coef, pred[c], *tables[c]))
            pred[c] = int(coef[0])
        bits = "".join(bits)
        bits += "1" * (-len(bits) % 8)
        for k in range(0, len(bits), 8):
            byte = int(bits[k:k + 8], 2)
            out.append(byte)
            if byte == 0xFF:
                out.append(0)
        if iv + 1 < intervals:
            out += bytes([0xFF, 0xD0 + iv % 8])
    out += bytes([0xFF, 0xD9])
    return bytes(out)


# ---- the reader: independent of everything above but ZIGZAG ----------------------------------------------------------------------

class _Bits:
    def __init__(self, data):
        self.data, self.pos, self.acc, self.n = data, 0, 0, 0

    def bit(self):
        if self.n == 0:
            b = self.data[self.pos]
            self.pos += 1
            if b == 0xFF:
                assert self.data[self.pos] == 0, "a marker inside an interval"
                self.pos += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v


def _lookup(bits, vals):
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[(length, code)] = vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return out


def _symbol(r, table):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | r.bit()
        if (length, code) in table:
            return table[(length, code)]
    raise AssertionError("no such Huffman code")


def _extend(v, size):
    return v if size == 0 or v >= (1 << (size - 1)) else v - (1 << size) + 1


def decode_coefficients(data):
    """Parses a baseline stream.  Returns a dict: height, width, markers (in order), quant {id: [64] natural order}, huffman
    {(class, id): (bits, vals)}, restart_interval (MCUs), sampling [(id, h, v, tq)], blocks: per component [n, 64] zigzag-ordered
    quantised coefficients in scan order, restarts: the RSTm numbers met, length: bytes up to and including EOI."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    info = {"markers": [0xD8], "quant": {}, "huffman": {}, "restart_interval": 0, "restarts": []}
    pos = 2
    while True:
        assert data[pos] == 0xFF, "a marker is expected at %d" % pos
        m = data[pos + 1]
        n = int.from_bytes(data[pos + 2:pos + 4], "big")
        seg = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        info["markers"].append(m)
        if m == 0xE0:
            info["app0"] = seg
        elif m == 0xDB:
            while seg:
                assert seg[0] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = list(seg[1:65])
                info["quant"][seg[0] & 15] = t
                seg = seg[65:]
        elif m == 0xC0:
            assert seg[0] == 8
            info["height"], info["width"] = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big")
            info["sampling"] = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])]
        elif m == 0xC4:
            while seg:
                bits = list(seg[1:17])
                info["huffman"][(seg[0] >> 4, seg[0] & 15)] = (bits, list(seg[17:17 + sum(bits)]))
                seg = seg[17 + sum(bits):]
        elif m == 0xDD:
            info["restart_interval"] = int.from_bytes(seg, "big")
        elif m == 0xDA:
            scan = [(seg[1 + 2 * i], seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(seg[0])]
            assert tuple(seg[1 + 2 * seg[0]:]) == (0, 63, 0)
            break
        else:
            raise AssertionError("marker %02x is not expected" % m)
    comps = info["sampling"]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mcux, mcuy = -(-info["width"] // (8 * hmax)), -(-info["height"] // (8 * vmax))
    tables = [(_lookup(*info["huffman"][(0, td)]), _lookup(*info["huffman"][(1, ta)])) for _, td, ta in scan]
    blocks = [[] for _ in comps]
    r, pred = _Bits(data[pos:]), [0] * len(comps)
    ri = info["restart_interval"]
    for mcu in range(mcux * mcuy):
        if ri and mcu and mcu % ri == 0:
            assert r.data[r.pos] == 0xFF and 0xD0 <= r.data[r.pos + 1] <= 0xD7, "a restart marker is expected"
            assert r.n == 0 or r.acc & ((1 << r.n) - 1) == (1 << r.n) - 1, "an interval is padded with 1-bits"
            info["restarts"].append(r.data[r.pos + 1] - 0xD0)
            r.pos, r.n, pred = r.pos + 2, 0, [0] * len(comps)
        for ci, (_, ch, cv, _) in enumerate(comps):
            for _ in range(ch * cv):
                coef = np.zeros(64, np.int64)
                size = _symbol(r, tables[ci][0])
                pred[ci] += _extend(r.bits(size), size)
                coef[0] = pred[ci]
                k = 1
                while k < 64:
                    s = _symbol(r, tables[ci][1])
                    run, size = s >> 4, s & 15
                    if size == 0:
                        if run != 15:
                            break
                        k += 16
                        continue
                    k += run
                    coef[k] = _extend(r.bits(size), size)
                    k += 1
                assert k <= 64
                blocks[ci].append(coef)
    assert r.n == 0 or r.acc & ((1 << r.n) - 1) == (1 << r.n) - 1, "the last interval is padded with 1-bits"
    end = pos + r.pos
    assert data[end:end + 2] == b"\xff\xd9", "EOI is expected behind the scan"
    info["length"] = end + 2
    info["blocks"] = [np.array(b) for b in blocks]
    info["mcus"] = (mcuy, mcux)
    return info


def reconstruct(info):
    """The float64 reconstruction of a decoded stream's component planes (extended size): dequantise, float IDCT, + 128, round, clamp."""
    from scipy.fft import idctn
    mcuy, mcux = info["mcus"]
    out = []
    for (cid, ch, cv, tq), blocks in zip(info["sampling"], info["blocks"]):
        q = info["quant"][tq]
        nat = np.zeros((len(blocks), 64))
        nat[:, ZIGZAG] = blocks
        px = np.clip(np.rint(idctn((nat * q).reshape(-1, 8, 8), axes=(1, 2), norm="ortho") + 128), 0, 255).astype(np.uint8)
        plane = np.zeros((mcuy * cv * 8, mcux * ch * 8), np.uint8)
        k = 0
        for my in range(mcuy):
            for mx in range(mcux):
                for i in range(cv):
                    for j in range(ch):
                        plane[(my * cv + i) * 8:(my * cv + i) * 8 + 8, (mx * ch + j) * 8:(mx * ch + j) * 8 + 8] = px[k]
                        k += 1
        out.append(plane)
    return out
