"""Host-side mirror of the reference's Python binding (raw_image_pipeline_python/src/
raw_image_pipeline_python.cpp:14-74: class ``RawImagePipeline``, 2 constructors, snake_case methods)
implemented over the C-ABI of ``librip_hip.so`` (include/rip.h) with ctypes.

All per-frame work runs in the HIP kernels of csrc/rip_{chain,stats,ccc,remap}.hip; this module only marshals
numpy / torch buffers.  It never falls back to a CPU implementation: a missing library or a
missing GPU raises.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librip_hip.so")

RIP_OK, RIP_ERR_INVALID_ARGUMENT, RIP_ERR_ASSERT, RIP_ERR_IO, RIP_ERR_DEVICE, RIP_ERR_CAPACITY = range(6)
TAP_DEBAYERED, TAP_COLOR, TAP_PROCESSED = 1, 2, 4
IMAGE_DEBAYERED, IMAGE_COLOR, IMAGE_PROCESSED, IMAGE_RECT_MASK = 0, 1, 2, 3


PACKED_SUFFIXES = {"10p": 10, "12p": 12, "10_csi2": 10, "12_csi2": 12}


def packed_bits(encoding):
    """Bits per sample of a packed Bayer encoding (bayer_<pattern>{10p,12p,10_csi2,12_csi2}, include/rip.h "Packed Bayer
    frames"), 0 for every other name."""
    if encoding.startswith("bayer_") and encoding[6:10] in ("rggb", "bggr", "gbrg", "grbg"):
        return PACKED_SUFFIXES.get(encoding[10:], 0)
    return 0


def packed_width(row_bytes, bits):
    """The pixels a tight packed row of ``row_bytes`` bytes holds: exact for tight rows of every width (the last byte of a
    row holds fewer than ``bits`` bits of padding); pitched rows need the width spelled out."""
    return 8 * int(row_bytes) // bits


# The output formats of set_output_format (include/rip.h rip_set_output_format) besides "native": numpy dtype of a delivered
# element, planar ([3, R, C]) or interleaved, channels.  numpy has no bfloat16: the host calls return bf16 as uint16 bit patterns.
OUTPUT_FORMATS = {
    "rgb8": (np.uint8, False, 3), "mono8": (np.uint8, False, 1),
    "rgb_chw_f32": (np.float32, True, 3), "rgb_chw_f16": (np.float16, True, 3), "rgb_chw_bf16": (np.uint16, True, 3),
    "bgr_chw_f32": (np.float32, True, 3), "bgr_chw_f16": (np.float16, True, 3), "bgr_chw_bf16": (np.uint16, True, 3),
}
# The YUV 4:2:0 formats, rows of the same shape: one channel of 3 H / 2 rows x W bytes that holds the three planes (yuv_planes takes it
# apart).  A table of its own: they are delivered like a native one-channel image -- uint8, [3 H / 2, W], no tensor dtype to pick --
# and the seeded draws of the suite's fuzzes are taken over OUTPUT_FORMATS as it stands.
YUV_OUTPUT_FORMATS = {"nv12": (np.uint8, False, 1), "i420": (np.uint8, False, 1)}
YUV_MATRICES = ("bt601", "bt709", "bt601_full", "bt709_full")
# The format "jpeg" (set_output_jpeg), a row of the same shape in a table of its own for the same reason: one channel, one row of
# `slot` bytes per frame, of which the first jpeg_sizes()[f] are frame f's stream (jpeg_streams cuts them out).
JPEG_OUTPUT_FORMATS = {"jpeg": (np.uint8, False, 1)}


def yuv_planes(frame, fmt):
    """(Y, Cb, Cr) views of a delivered "nv12" / "i420" frame: a numpy array or torch tensor of shape [3 H / 2, W] (or with leading
    batch axes).  Y is [H, W], Cb and Cr are [H / 2, W / 2]; under "nv12" they are strided views of the interleaved chroma rows,
    under "i420" views of the two contiguous planes behind Y.  ``frame`` must hold tightly packed rows (what the host calls and
    ``apply_device`` without ``out`` return)."""
    if fmt not in ("nv12", "i420"):
        raise ValueError("yuv_planes: 'nv12' or 'i420', got %r" % (fmt,))
    rows, w = frame.shape[-2], frame.shape[-1]
    if rows % 3 or w % 2:
        raise ValueError("yuv_planes: a [3 H / 2, W] frame with even H and W is expected, got %s" % (tuple(frame.shape),))
    h = rows // 3 * 2
    y, c = frame[..., :h, :], frame[..., h:, :]
    if fmt == "nv12":
        return y, c[..., 0::2], c[..., 1::2]
    lead = tuple(frame.shape[:-2])
    planes = c.reshape(lead + (2, h // 2, w // 2))  # h / 2 rows of w bytes are h / 2 rows of w / 2 bytes twice
    return y, planes[..., 0, :, :], planes[..., 1, :, :]


def jpeg_streams(slots, sizes):
    """The streams of delivered "jpeg" frames as a list of ``bytes``: ``slots`` is the [n, slot] uint8 array or tensor ``apply_device``
    returned (any row stride), ``sizes`` the n lengths of ``jpeg_sizes()``.  A frame whose stream did not fit its slot has size 0 and
    gives ``b""``."""
    if len(sizes) != slots.shape[0]:
        raise ValueError("jpeg_streams: %d sizes for %d slots" % (len(sizes), slots.shape[0]))
    host = slots.cpu().numpy() if hasattr(slots, "cpu") else np.asarray(slots)
    return [host[f, :int(s)].tobytes() for f, s in enumerate(sizes)]


def _delivered(rows, cols, channels, encoding):
    """(shape, numpy dtype) of one delivered frame as rip_query_output / rip_apply / rip_collect describe it."""
    dtype, planar, _ = OUTPUT_FORMATS.get(encoding, (np.uint16 if encoding.endswith("16") else np.uint8, False, channels))
    if planar:
        return (channels, rows, cols), np.dtype(dtype)
    return ((rows, cols) if channels == 1 else (rows, cols, channels)), np.dtype(dtype)


class _HeadBuffer(C.Structure):
    """rip_head_buffer (include/rip.h)."""
    _fields_ = [("d_out", C.c_void_p), ("out_step", C.c_size_t), ("out_frame_stride", C.c_size_t)]


class RipError(RuntimeError):
    """HIP/device failure (RIP_ERR_DEVICE, RIP_ERR_CAPACITY)."""


class RipAssertError(RipError):
    """Input the reference's OpenCV call would have asserted on (cv::Exception)."""


class RipIOError(RipError, IOError):
    """Malformed YAML / model file (YAML::Exception class of failures)."""


_lib = None


def load_library(path=None):
    """Loads librip_hip.so.  Raises if it has not been built (``python -m raw_image_pipeline_amd.build``
    or ``__graft_entry__.build()``): there is no other implementation to fall back to."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("RIP_LIBRARY") or LIB_PATH  # RIP_LIBRARY: A/B runs of two builds on one GPU box
    try:
        # torch bundles its own libamdhip64 (same soname as ROCm's): import it first so that this
        # library binds to the SAME HIP runtime -- device pointers and streams are shared with torch.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise RuntimeError("%s is missing: build it with `python raw_image_pipeline_amd/build.py` "
                           "(hipcc, gfx950). The pipeline has no CPU fallback." % path)
    lib = C.CDLL(path)
    lib.rip_last_error.restype = C.c_char_p
    lib.rip_last_error.argtypes = [C.c_void_p]
    lib.rip_version.restype = C.c_char_p
    lib.rip_destroy.restype = None
    lib.rip_destroy.argtypes = [C.c_void_p]
    lib.rip_copy_host.restype = None
    lib.rip_copy_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    _lib = lib
    return lib


def _as_doubles(values, n=None):
    arr = (C.c_double * len(values))(*[float(v) for v in values])
    return arr, len(values)


def _wrap_pinned(raw, shape, dtype):
    """THE array over a ctypes byte buffer: built in one step, so that its ``base`` is the buffer object and not another
    ndarray.  numpy collapses the base chain of a view through every non-owning ndarray until it meets something that is not
    one: a slice / reshape / reversed view of this array therefore references THIS array -- the object the ``OutputPool``
    counts references of.  (Until round 5 this was ``np.frombuffer(raw).reshape(shape)``: views of the reshaped array
    referenced the hidden frombuffer array, the pool saw no reference and recycled page-locked memory a caller's slice still
    looked at -- ADVICE round 4.)"""
    return np.ndarray(tuple(shape), dtype=np.dtype(dtype), buffer=raw)


def host_alloc(shape, dtype=np.uint8):
    """A numpy array over page-locked host memory (rip_host_alloc): frames handed to ``submit`` from it are uploaded
    asynchronously without the staging copy a pageable frame gets -- and must stay untouched until their ``collect``.
    The memory is released with the array."""
    import weakref
    lib = load_library()
    lib.rip_host_alloc.restype = C.c_void_p
    lib.rip_host_alloc.argtypes = [C.c_size_t]
    lib.rip_host_free.restype = None
    lib.rip_host_free.argtypes = [C.c_void_p]
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    ptr = lib.rip_host_alloc(max(n, 1))
    if not ptr:
        raise MemoryError("rip_host_alloc(%d) failed" % n)
    raw = (C.c_uint8 * max(n, 1)).from_address(ptr)
    weakref.finalize(raw, lib.rip_host_free, C.c_void_p(ptr))  # the ctypes object is the base of every view below
    return _wrap_pinned(raw, shape, dtype)


class OutputPool:
    """Destination arrays for the deep copies a pipeline hands out (``RawImagePipeline.out_pool``).  A fresh 15 MB numpy
    array costs more than filling it -- the kernel zeroes every new page -- so the pool keeps the arrays it has handed out
    and hands one out again once NOBODY else references it any more (CPython reference count: only the pool's own list
    holds it; a view of an array keeps its base alive and therefore counts).  The caller still owns what it gets, for as long
    as it keeps it: an array in use is never recycled.  At most ``limit`` arrays per shape are remembered."""

    def __init__(self, limit=8, pinned=False):
        self.limit = int(limit)
        self.pinned = bool(pinned)  # page-locked arrays (host_alloc): ``submit(..., out=...)`` downloads straight into them
        self._arrays = {}
        self._refcount = getattr(sys, "getrefcount", None)

    def take(self, shape, dtype=np.uint8, or_none=False):
        """An array of this shape nobody else references.  A pinned pool whose ``limit`` arrays are all in use hands out an
        ordinary array (page-locked memory is only worth its allocation when it is recycled) -- or None with ``or_none``,
        for callers that need the page lock (``submit(..., out=)``)."""
        key = (tuple(shape), np.dtype(dtype).str)
        if key not in self._arrays and len(self._arrays) >= 4:
            # a camera whose image size keeps changing must not pile up page-locked memory: forget the arrays of the shapes
            # seen longest ago (whoever still holds one of them keeps it alive; it just is not recycled any more)
            for old in list(self._arrays)[:len(self._arrays) - 3]:
                del self._arrays[old]
        arrays = self._arrays.pop(key, [])
        self._arrays[key] = arrays  # most recently used last
        if self._refcount is not None:
            for i in range(len(arrays)):
                # references: the list, the call argument of getrefcount -- anything above is somebody else's
                if self._refcount(arrays[i]) == 2:
                    return arrays[i]
        if self.pinned and not (self._refcount is not None and len(arrays) < self.limit):
            return None if or_none else np.empty(shape, dtype)
        arr = host_alloc(shape, dtype) if self.pinned else np.empty(shape, dtype)
        if self._refcount is not None and len(arrays) < self.limit:
            arrays.append(arr)
        return arr


class LaunchLog:
    """The launch record of a pipeline handle (RawImagePipeline.launch_log): one line per kernel launch,
    ``<kernel> fc=<0|1> grid=<x>,<y> block=<n> frames=<n>``."""

    def __init__(self, pipe):
        self._pipe = pipe
        self.text = ""

    def __enter__(self):
        self._pipe._call("rip_debug_launch_log", 1)
        return self

    def __exit__(self, *exc):
        self.text = self._pipe._launch_log_text()
        self._pipe._call("rip_debug_launch_log", 0)
        return False

    def records(self):
        """[{"name", "fc", "grid": (x, y), "block", "frames"}] in launch order (also inside the block)."""
        out = []
        for line in (self.text or self._pipe._launch_log_text()).splitlines():
            name, rest = line.split(" fc=", 1)
            f = dict(kv.split("=") for kv in ("fc=" + rest).split())
            out.append({"name": name, "fc": int(f["fc"]), "grid": tuple(int(v) for v in f["grid"].split(",")),
                        "block": int(f["block"]), "frames": int(f["frames"])})
        return out

    def names(self):
        return [r["name"] for r in self.records()]

    def keys(self):
        """{(name, fc)} of the launches."""
        return {(r["name"], r["fc"]) for r in self.records()}


class RawImagePipeline:
    """Same surface as ``py_raw_image_pipeline.RawImagePipeline``.

    ``RawImagePipeline(use_gpu)`` mirrors the one-argument constructor (example params, example
    camera and colour calibration); ``RawImagePipeline(use_gpu, params_path, calibration_path,
    color_calibration_path)`` the four-argument one.  ``use_gpu`` is recorded only: every stage
    always runs on the MI355X and follows the reference's CPU/OpenCV arithmetic.
    """

    _ONE_ARG = object()

    def __init__(self, use_gpu=False, params_path=_ONE_ARG, calibration_path="", color_calibration_path="",
                 device=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        self.last_encoding = None
        if params_path is RawImagePipeline._ONE_ARG:
            st = self._lib.rip_create_default(int(device), int(bool(use_gpu)), C.byref(self._h))
        else:
            st = self._lib.rip_create(int(device), int(bool(use_gpu)), (params_path or "").encode(),
                                      (calibration_path or "").encode(), (color_calibration_path or "").encode(),
                                      C.byref(self._h))
        if st != RIP_OK:
            msg = self._lib.rip_last_error(None).decode(errors="replace")
            self._h = C.c_void_p()
            self._raise(st, msg)
        self.device = int(device)
        self._torch_stream = None
        self.out_pool = None  # an OutputPool: collect() / the image getters then recycle the arrays of their deep copies
        self._given = {}       # ticket -> (out, tap_debayered, tap_color) arrays handed to submit()
        self._given_last = (None, None, None)  # ... of the frame collected last (what the image getters return)
        self._output_format = self.get_output_format()  # kept beside the handle's: apply_device asks on every batch

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.rip_destroy(h)
            self._h = C.c_void_p()

    close = __del__

    # ---- plumbing ------------------------------------------------------------------------------
    @staticmethod
    def _raise(st, msg):
        if st == RIP_ERR_INVALID_ARGUMENT:
            raise ValueError(msg)  # std::invalid_argument
        if st == RIP_ERR_ASSERT:
            raise RipAssertError(msg)
        if st == RIP_ERR_IO:
            raise RipIOError(msg)
        raise RipError(msg)

    def _check(self, st):
        if st != RIP_OK:
            self._raise(st, self._lib.rip_last_error(self._h).decode(errors="replace"))  # a message may quote bytes of a malformed file

    def _call(self, name, *args):
        self._check(getattr(self._lib, name)(self._h, *args))

    def set_stream(self, stream):
        """HIP stream handle (int / torch.cuda.Stream) the device work is enqueued on."""
        self._torch_stream = stream if hasattr(stream, "wait_stream") else None
        handle = getattr(stream, "cuda_stream", stream)
        self._call("rip_set_stream", C.c_void_p(int(handle) if handle else 0))

    # ---- frame API -------------------------------------------------------------------------------
    def query_output(self, rows, cols, channels, encoding):
        r, c, cn = C.c_int(), C.c_int(), C.c_int()
        enc = C.create_string_buffer(32)
        self._call("rip_query_output", int(rows), int(cols), int(channels), encoding.encode(), C.byref(r), C.byref(c),
                   C.byref(cn), enc)
        return r.value, c.value, cn.value, enc.value.decode()

    def query_output_bytes(self, rows, cols, channels, encoding):
        """(bytes, element bytes, planar) of one tightly packed delivered frame (rip_query_output_bytes): what the capacities
        of ``process`` / ``submit(out=)`` / ``collect`` are checked against."""
        b, e, pl = C.c_size_t(), C.c_int(), C.c_int()
        self._call("rip_query_output_bytes", int(rows), int(cols), int(channels), encoding.encode(), C.byref(b), C.byref(e), C.byref(pl))
        return b.value, e.value, bool(pl.value)

    def query_taps(self, rows, cols, channels, encoding):
        """Geometry of the debayered / colour taps (post-flip, pre-undistortion): rows, cols, channels."""
        tr, tc, tcn = C.c_int(), C.c_int(), C.c_int()
        self._call("rip_query_taps", int(rows), int(cols), int(channels), encoding.encode(), C.byref(tr), C.byref(tc), C.byref(tcn))
        return tr.value, tc.value, tcn.value

    @staticmethod
    def _packed_geometry(img, encoding, width):
        """(rows, cols, channels) of a host frame: for the packed Bayer encodings a 2-D uint8 array [rows, row bytes] whose
        pixel count per row is ``width`` (default: what a tight row of that many bytes holds)."""
        bits = packed_bits(encoding)
        if not bits:
            if width is not None:
                raise ValueError("width is for the packed Bayer encodings only")
            return img.shape[0], img.shape[1], 1 if img.ndim == 2 else img.shape[2]
        if img.dtype != np.uint8 or img.ndim != 2:
            raise ValueError("a %s frame is a 2-D uint8 array [rows, row bytes]" % encoding)
        cols = packed_width(img.shape[1], bits) if width is None else int(width)
        if (cols * bits + 7) // 8 > img.shape[1]:
            raise ValueError("rows of %d bytes do not hold %d pixels of %d bits" % (img.shape[1], cols, bits))
        return img.shape[0], cols, 1

    def process(self, image, encoding, width=None):
        """cv::Mat process(const cv::Mat&, std::string&): returns a new array; input untouched.  Packed Bayer encodings
        (bayer_*10p / 12p / 10_csi2 / 12_csi2): ``image`` is the 2-D uint8 array [rows, row bytes], ``width`` the pixels per row
        (default ``8 * row_bytes // bits``: exact for tight rows; pass it for pitched ones)."""
        img = np.asarray(image)
        # 16-bit Bayer extension (set_debayer_16bit): uint16 in; uint16 BGR out, or -- with a 16-bit range
        # (set_debayer_16bit_range) -- the whole pipeline and uint8 bgr8 out
        wide = img.dtype == np.uint16
        if img.dtype not in (np.uint8, np.uint16) or img.ndim not in (2, 3):
            raise ValueError("image must be uint8 (or uint16 Bayer), HxW or HxWxC")
        if img.strides[-1] != img.itemsize or (img.ndim == 3 and img.strides[1] != img.shape[2] * img.itemsize):
            img = np.ascontiguousarray(img)
        rows, cols, cn = self._packed_geometry(img, encoding, width)
        orows, ocols, ocn, oenc = self.query_output(rows, cols, cn, encoding)
        if wide != encoding.endswith("16"):
            raise ValueError("dtype %s does not match encoding %s" % (img.dtype, encoding))
        oshape, odtype = _delivered(orows, ocols, ocn, oenc)
        out = self.out_pool.take(oshape, odtype) if self.out_pool is not None else np.empty(oshape, odtype)
        r, c, k = C.c_int(), C.c_int(), C.c_int()
        enc = C.create_string_buffer(32)
        self._given_last = (None, None, None)  # the image getters now belong to this frame
        self._call("rip_apply", img.ctypes.data_as(C.c_void_p), rows, cols, cn, C.c_size_t(img.strides[0]),
                   encoding.encode(), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes), C.byref(r), C.byref(c),
                   C.byref(k), enc)
        self.last_encoding = enc.value.decode()
        shape, _ = _delivered(r.value, c.value, k.value, self.last_encoding)
        if self.last_encoding == "jpeg":  # one slot: the stream is its first jpeg_sizes()[0] bytes, the only ones downloaded
            return out.reshape(-1)[:int(self.jpeg_sizes()[0])]
        return out if out.shape == shape else out.reshape(shape)

    def apply(self, image, encoding, width=None):
        """bool apply(cv::Mat&, std::string&): returns the processed image; when it has the input's
        shape the input array is overwritten too (the reference re-seats the caller's Mat)."""
        out = self.process(image, encoding, width)
        if isinstance(image, np.ndarray) and image.shape == out.shape and image.flags.writeable:
            image[...] = out
        return out

    # ---- asynchronous host frames (rip_submit / rip_collect; no counterpart in the reference's binding) -------------
    def submit(self, image, encoding, out=None, tap_debayered=None, tap_color=None, width=None):
        """Enqueues upload + chain + download of one host frame and returns its ticket without waiting (rip_submit).  Up to
        ``set_ring_depth`` (default 3) frames may be in flight; frames are processed in submission order.

        ``out`` / ``tap_debayered`` / ``tap_color``: page-locked arrays (``host_alloc``, a pinned ``OutputPool``) of the
        result's / the taps' shape -- the downloads are written straight into them (rip_submit_to) and ``collect`` / the image
        getters return these very arrays: deep-copy semantics without a copy.  ``width``: as for ``process``."""
        img = np.asarray(image)
        if img.dtype not in (np.uint8, np.uint16) or img.ndim not in (2, 3):
            raise ValueError("image must be uint8 (or uint16 Bayer), HxW or HxWxC")
        if img.strides[-1] != img.itemsize or (img.ndim == 3 and img.strides[1] != img.shape[2] * img.itemsize):
            img = np.ascontiguousarray(img)
        rows, cols, cn = self._packed_geometry(img, encoding, width)
        if (img.dtype == np.uint16) != encoding.endswith("16"):
            raise ValueError("dtype %s does not match encoding %s" % (img.dtype, encoding))
        t = C.c_uint64()
        given = (out, tap_debayered, tap_color)
        if all(g is None for g in given):
            self._call("rip_submit", img.ctypes.data_as(C.c_void_p), rows, cols, cn, C.c_size_t(img.strides[0]), encoding.encode(), C.byref(t))
            return t.value
        for g in given:
            if g is not None and not (isinstance(g, np.ndarray) and g.flags.c_contiguous and g.flags.writeable):
                raise ValueError("out / tap arrays must be writeable C-contiguous numpy arrays over page-locked memory")
        ptr = lambda g: g.ctypes.data_as(C.c_void_p) if g is not None else None
        taps = [g for g in (tap_debayered, tap_color) if g is not None]
        self._call("rip_submit_to", img.ctypes.data_as(C.c_void_p), rows, cols, cn, C.c_size_t(img.strides[0]), encoding.encode(),
                   ptr(out), C.c_size_t(out.nbytes if out is not None else 0), ptr(tap_debayered), ptr(tap_color),
                   C.c_size_t(min(g.nbytes for g in taps) if taps else 0), C.byref(t))
        self._given[t.value] = given
        return t.value

    def collect(self, ticket, copy=True):
        """Waits for the frame of ``ticket`` and returns its image (rip_collect).  ``copy=False`` returns a read-only view of
        the handle's pinned result buffer instead.  As rip.h says of rip_collect's view: it is valid until the NEXT ``collect``
        on this pipeline -- or until a ``submit`` finds every other slot in flight and takes this one (keep at most
        ``ring depth - 1`` frames in flight to hold on to a view while submitting); copy what must live longer."""
        r, c, k = C.c_int(), C.c_int(), C.c_int()
        enc = C.create_string_buffer(32)
        view = C.c_void_p()
        self._call("rip_collect", C.c_uint64(int(ticket)), None, C.c_size_t(0), C.byref(view), C.byref(r), C.byref(c), C.byref(k), enc)
        self.last_encoding = enc.value.decode()
        shape, dtype = _delivered(r.value, c.value, k.value, self.last_encoding)
        n = r.value * c.value * k.value
        self._given_last = self._given.pop(int(ticket), (None, None, None))
        if self._given_last[0] is not None:  # the download went straight into the caller's array: it IS the deep copy
            g = self._given_last[0]
            return g if g.shape == tuple(shape) else g.reshape(shape)
        if copy:  # the library's copy (split over a few threads for whole frames), not numpy's
            out = self.out_pool.take(shape, dtype) if self.out_pool is not None else np.empty(shape, dtype)
            self._lib.rip_copy_host(out.ctypes.data_as(C.c_void_p), view, C.c_size_t(out.nbytes))
            return out
        buf = C.c_uint8 * (n * dtype.itemsize)
        arr = np.frombuffer(buf.from_address(view.value), dtype).reshape(shape)
        arr.flags.writeable = False
        return arr

    def set_ring_depth(self, depth):
        self._call("rip_set_ring_depth", int(depth))

    @staticmethod
    def _device_frames_geometry(frames, encoding, width):
        """(n, rows, cols, channels, row pitch, frame stride) of a device batch as apply_device takes it."""
        import torch
        if frames.dtype != torch.uint8 or not frames.is_cuda:
            raise ValueError("frames must be a uint8 CUDA tensor")
        wide = encoding.endswith("16")
        bits = packed_bits(encoding)
        if width is not None and not bits:
            raise ValueError("width is for the packed Bayer encodings only")
        if bits:
            if frames.dim() != 3:
                raise ValueError("packed frames must be [n, rows, row bytes]")
            n, rows = frames.shape[0], frames.shape[1]
            cols = packed_width(frames.shape[2], bits) if width is None else int(width)
            if (cols * bits + 7) // 8 > frames.shape[2]:
                raise ValueError("rows of %d bytes do not hold %d pixels of %d bits" % (frames.shape[2], cols, bits))
            cn = 1
        elif wide:
            if frames.dim() != 3 or frames.shape[2] % 2:
                raise ValueError("16-bit frames must be the uint8 view [n, rows, cols * 2] of uint16 rows")
            n, rows, cols = frames.shape[0], frames.shape[1], frames.shape[2] // 2
            cn = 1
        elif frames.dim() == 3:
            n, rows, cols = frames.shape
            cn = 1
        elif frames.dim() == 4:
            n, rows, cols, cn = frames.shape
        else:
            raise ValueError("frames must be [n, rows, cols] or [n, rows, cols, c]")
        if frames.stride(-1) != 1 or (frames.dim() == 4 and frames.stride(2) != cn):
            raise ValueError("pixels must be contiguous")
        in_step = frames.stride(1)
        in_frame = frames.stride(0) if n > 1 else in_step * rows
        return n, rows, cols, cn, in_step, in_frame

    def apply_device(self, frames, encoding, out=None, tap_debayered=None, tap_color=None, width=None):
        """Device-resident batch (rip_apply_device).  ``frames``: uint8 CUDA tensor [n, rows, cols]
        or [n, rows, cols, c] (torch) already in HBM; returns the output tensor [n, R, C(, 3)].
        Asynchronous on the handle's stream.

        bayer_*16 frames (``set_debayer_16bit``): the uint8 view [n, rows, cols * 2] of the uint16 rows, pitches in bytes.
        With a 16-bit range (``set_debayer_16bit_range``) the result is the ordinary uint8 [n, R, C, 3] tensor and taps may be
        given; without one it is bgr16 as bytes, [n, R, C, 6].

        Packed Bayer encodings: [n, rows, row bytes] uint8 tensors, ``width`` pixels per row (default
        ``8 * row_bytes // bits``); the result is the ordinary uint8 [n, R, C, 3] tensor and taps may be given.

        Under an output format (``set_output_format``) the result is uint8 [n, R, C, 3] (rgb8) / [n, R, C] (mono8) or float32 /
        float16 / bfloat16 [n, 3, R, C]; ``out`` may then be a strided view whose innermost elements are contiguous: its row
        pitch and frame stride are handed on as rip_apply_device's out_step / out_frame_stride (a planar view's planes must lie
        ``rows`` row pitches apart)."""
        import torch
        n, rows, cols, cn, in_step, in_frame = self._device_frames_geometry(frames, encoding, width)
        orows, ocols, ocn, enc = self.query_output(rows, cols, cn, encoding)
        out_step = out_frame = 0
        if self._output_format != "native" and enc in OUTPUT_FORMATS:
            dtype, planar, _ = OUTPUT_FORMATS[enc]
            tdtype = torch.bfloat16 if enc.endswith("bf16") else {np.uint8: torch.uint8, np.float32: torch.float32, np.float16: torch.float16}[dtype]
            shape = (n, 3, orows, ocols) if planar else ((n, orows, ocols) if ocn == 1 else (n, orows, ocols, ocn))
            if out is None:
                out = torch.empty(shape, dtype=tdtype, device=frames.device)
            elif tuple(out.shape) != shape or out.dtype != tdtype:
                raise ValueError("out must be a %s tensor of shape %s" % (tdtype, shape))
            elif not out.is_contiguous():
                elem = out.element_size()
                ok = out.stride(-1) == 1 and (planar or ocn == 1 or out.stride(2) == ocn) and (not planar or out.stride(1) == out.stride(2) * orows)
                if not ok:
                    raise ValueError("out: the elements of a row must be contiguous and the planes of a frame `rows` row pitches apart")
                out_step = out.stride(2 if planar else 1) * elem
                out_frame = out.stride(0) * elem if n > 1 else 0
        elif enc == "jpeg":  # one slot per frame: [n, slot]; a given tensor's width is the slot the caller chose, its row stride the frame stride
            if out is None:
                out = torch.empty((n, ocols), dtype=torch.uint8, device=frames.device)
            elif out.dim() != 2 or out.shape[0] != n or out.dtype != torch.uint8 or out.stride(1) != 1:
                raise ValueError("out must be a uint8 tensor [%d, slot] with contiguous rows" % n)
            out_step = out.shape[1]
            out_frame = out.stride(0) if n > 1 else 0
        else:
            shape = (n, orows, ocols) if ocn == 1 else (n, orows, ocols, ocn * (2 if enc.endswith("16") else 1))
            if out is None:
                out = torch.empty(shape, dtype=torch.uint8, device=frames.device)
            elif tuple(out.shape) != shape or not out.is_contiguous():
                raise ValueError("out must be a contiguous tensor of shape %s" % (shape,))
        if out.device != frames.device:
            raise ValueError("out must live on the device of frames")
        # taps hold the post-flip, pre-undistortion geometry (tightly packed): query it with undistortion off
        if tap_debayered is not None or tap_color is not None:
            tr, tc, tcn = C.c_int(), C.c_int(), C.c_int()
            self._call("rip_query_taps", int(rows), int(cols), int(cn), encoding.encode(), C.byref(tr), C.byref(tc), C.byref(tcn))
            tshape = (n, tr.value, tc.value) if tcn.value == 1 else (n, tr.value, tc.value, tcn.value)
            for t in (tap_debayered, tap_color):
                if t is not None and (t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tshape
                                      or t.device != frames.device):
                    raise ValueError("tap tensors must be contiguous uint8 CUDA tensors of shape %s" % (tshape,))
        # The C call enqueues on the handle's stream; the tensors were produced / allocated on torch's current stream.
        # Order the two when they differ, and tell the caching allocator that the handle's stream uses the buffers.
        cur = torch.cuda.current_stream(frames.device)
        mine = self._torch_stream
        if mine is not None and mine.cuda_stream != cur.cuda_stream:
            mine.wait_stream(cur)
            for t in (frames, out, tap_debayered, tap_color):
                if t is not None:
                    t.record_stream(mine)
        with torch.cuda.device(frames.device):  # the C-ABI selects the handle's device; keep the caller's current device
            self._given_last = (None, None, None)
            self._call("rip_apply_device", C.c_void_p(frames.data_ptr()), C.c_size_t(in_step), C.c_size_t(in_frame), int(n),
                       int(rows), int(cols), int(cn), encoding.encode(), C.c_void_p(out.data_ptr()), C.c_size_t(out_step),
                       C.c_size_t(out_frame), C.c_void_p(tap_debayered.data_ptr() if tap_debayered is not None else 0),
                       C.c_void_p(tap_color.data_ptr() if tap_color is not None else 0))
        self.last_encoding = enc
        return out

    # ---- output heads (rip_set_output_heads; no counterpart in the reference's binding) -------------------------------
    def set_output_heads(self, n):
        """How many output heads the handle has, 1..8 (include/rip.h rip_set_output_heads): each is one complete set of the output
        settings; heads at and beyond ``n`` go back to the defaults and a selection at or beyond ``n`` becomes 0."""
        self._call("rip_set_output_heads", int(n))
        self._output_format = self.get_output_format()

    def get_output_heads(self):
        n = C.c_int()
        self._call("rip_get_output_heads", C.byref(n))
        return n.value

    def select_output_head(self, head):
        """The head every single-output setter, getter, query and frame call addresses from now on (rip_select_output_head)."""
        self._call("rip_select_output_head", int(head))
        self._output_format = self.get_output_format()

    def get_selected_output_head(self):
        h = C.c_int()
        self._call("rip_get_selected_output_head", C.byref(h))
        return h.value

    def debug_output_head_info(self, head):
        """(table builds, direct write, copied) of a head (rip_debug_output_head_info)."""
        b, d, c = C.c_int(), C.c_int(), C.c_int()
        self._call("rip_debug_output_head_info", int(head), C.byref(b), C.byref(d), C.byref(c))
        return b.value, d.value, c.value

    def _head_queries(self, heads, rows, cols, cn, encoding):
        """query_output of every head in ``heads`` (None elsewhere), each under its own selection; the selection is put back."""
        n = self.get_output_heads()
        was = self.get_selected_output_head()
        info = [None] * n
        try:
            for k in heads:
                self._call("rip_select_output_head", int(k))
                try:
                    info[k] = self.query_output(rows, cols, cn, encoding) + (self.get_output_format(),)
                except (ValueError, RipError) as e:  # named as the heads calls of the C ABI name it
                    raise type(e)("output head %d: %s" % (k, e)) from None
        finally:
            self._call("rip_select_output_head", was)
        return info

    def apply_device_heads(self, frames, encoding, heads=None, outs=None, tap_debayered=None, tap_color=None, width=None):
        """Device-resident batch, one result per requested output head from one run of the chain (rip_apply_device_heads).
        ``heads``: the indices to deliver (default: all); ``outs``: a list with one entry per head of the handle, a tensor to
        write into or None.  Returns a list with one tensor per head, None for heads not requested; dtype and shape of each
        follow ``apply_device``'s rules for that head's settings.  A given tensor may be a strided view whose innermost elements
        are contiguous (planes of a planar view ``rows`` row pitches apart)."""
        import torch
        n, rows, cols, cn, in_step, in_frame = self._device_frames_geometry(frames, encoding, width)
        n_heads = self.get_output_heads()
        wanted = sorted(set(range(n_heads) if heads is None else [int(k) for k in heads]))
        if not wanted or wanted[0] < 0 or wanted[-1] >= n_heads:
            raise ValueError("heads must name at least one of the handle's heads 0..%d" % (n_heads - 1))
        if outs is not None and len(outs) != n_heads:
            raise ValueError("outs must have one entry per head of the handle (%d)" % n_heads)
        info = self._head_queries(wanted, rows, cols, cn, encoding)
        result = [None] * n_heads
        bufs = (_HeadBuffer * n_heads)()
        for k in wanted:
            orows, ocols, ocn, enc, fmt = info[k]
            out = outs[k] if outs is not None else None
            if fmt != "native" and enc in OUTPUT_FORMATS:
                dtype, planar, _ = OUTPUT_FORMATS[enc]
                tdtype = torch.bfloat16 if enc.endswith("bf16") else {np.uint8: torch.uint8, np.float32: torch.float32, np.float16: torch.float16}[dtype]
                shape = (n, 3, orows, ocols) if planar else ((n, orows, ocols) if ocn == 1 else (n, orows, ocols, ocn))
            else:
                planar, tdtype = False, torch.uint8
                shape = (n, orows, ocols) if ocn == 1 else (n, orows, ocols, ocn * (2 if enc.endswith("16") else 1))
            out_step = out_frame = 0
            if enc == "jpeg":  # apply_device's rule: [n, slot], a given tensor's width is its slot
                if out is None:
                    out = torch.empty((n, ocols), dtype=torch.uint8, device=frames.device)
                elif out.dim() != 2 or out.shape[0] != n or out.dtype != torch.uint8 or out.stride(1) != 1 or out.device != frames.device:
                    raise ValueError("outs[%d] must be a uint8 tensor [%d, slot] with contiguous rows on the device of frames" % (k, n))
                out_step = out.shape[1]
                out_frame = out.stride(0) if n > 1 else 0
            elif out is None:
                out = torch.empty(shape, dtype=tdtype, device=frames.device)
            elif tuple(out.shape) != shape or out.dtype != tdtype or out.device != frames.device:
                raise ValueError("outs[%d] must be a %s tensor of shape %s on the device of frames" % (k, tdtype, shape))
            elif not out.is_contiguous():
                elem = out.element_size()
                inner = len(shape) == 4 and not planar
                ok = out.stride(-1) == 1 and (not inner or out.stride(2) == shape[3]) and (not planar or out.stride(1) == out.stride(2) * orows)
                if not ok:
                    raise ValueError("outs[%d]: the elements of a row must be contiguous and the planes of a frame `rows` row pitches apart" % k)
                out_step = out.stride(2 if planar else 1) * elem
                out_frame = out.stride(0) * elem if n > 1 else 0
            result[k] = out
            bufs[k] = _HeadBuffer(C.c_void_p(out.data_ptr()), out_step, out_frame)
        if tap_debayered is not None or tap_color is not None:
            tr, tc, tcn = self.query_taps(rows, cols, cn, encoding)
            tshape = (n, tr, tc) if tcn == 1 else (n, tr, tc, tcn)
            for t in (tap_debayered, tap_color):
                if t is not None and (t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tshape
                                      or t.device != frames.device):
                    raise ValueError("tap tensors must be contiguous uint8 CUDA tensors of shape %s" % (tshape,))
        cur = torch.cuda.current_stream(frames.device)
        mine = self._torch_stream
        if mine is not None and mine.cuda_stream != cur.cuda_stream:
            mine.wait_stream(cur)
            for t in [frames, tap_debayered, tap_color] + result:
                if t is not None:
                    t.record_stream(mine)
        with torch.cuda.device(frames.device):
            self._given_last = (None, None, None)
            self._call("rip_apply_device_heads", C.c_void_p(frames.data_ptr()), C.c_size_t(in_step), C.c_size_t(in_frame), int(n),
                       int(rows), int(cols), int(cn), encoding.encode(), bufs, int(n_heads),
                       C.c_void_p(tap_debayered.data_ptr() if tap_debayered is not None else 0),
                       C.c_void_p(tap_color.data_ptr() if tap_color is not None else 0))
        return result

    def apply_heads(self, image, encoding, heads=None, width=None):
        """One host frame, one result per requested output head from one upload and one run of the chain (rip_apply_heads).
        Returns a list with one numpy array per head of the handle (None for heads not requested), each of the shape and dtype
        ``process`` returns under that head's settings.  The image getters keep the taps; there is no processed image."""
        img = np.asarray(image)
        if img.dtype not in (np.uint8, np.uint16) or img.ndim not in (2, 3):
            raise ValueError("image must be uint8 (or uint16 Bayer), HxW or HxWxC")
        if img.strides[-1] != img.itemsize or (img.ndim == 3 and img.strides[1] != img.shape[2] * img.itemsize):
            img = np.ascontiguousarray(img)
        rows, cols, cn = self._packed_geometry(img, encoding, width)
        if (img.dtype == np.uint16) != encoding.endswith("16"):
            raise ValueError("dtype %s does not match encoding %s" % (img.dtype, encoding))
        n_heads = self.get_output_heads()
        wanted = sorted(set(range(n_heads) if heads is None else [int(k) for k in heads]))
        if not wanted or wanted[0] < 0 or wanted[-1] >= n_heads:
            raise ValueError("heads must name at least one of the handle's heads 0..%d" % (n_heads - 1))
        info = self._head_queries(wanted, rows, cols, cn, encoding)
        result = [None] * n_heads
        ptrs, caps = (C.c_void_p * n_heads)(), (C.c_size_t * n_heads)()
        for k in wanted:
            shape, dtype = _delivered(*info[k][:4])
            result[k] = np.empty(shape, dtype)
            ptrs[k], caps[k] = result[k].ctypes.data, result[k].nbytes
        r, c, ch = (C.c_int * n_heads)(), (C.c_int * n_heads)(), (C.c_int * n_heads)()
        self._given_last = (None, None, None)
        self._call("rip_apply_heads", img.ctypes.data_as(C.c_void_p), rows, cols, cn, C.c_size_t(img.strides[0]), encoding.encode(),
                   ptrs, caps, int(n_heads), r, c, ch)
        for k in wanted:
            assert (r[k], c[k], ch[k]) == info[k][:3]
            if info[k][3] == "jpeg":  # the stream: the first jpeg_sizes()[0] bytes of the slot, the only ones downloaded
                result[k] = result[k].reshape(-1)[:int(self.jpeg_sizes(head=k)[0])]
        return result

    def set_taps(self, mask):
        self._call("rip_set_taps", int(mask))

    def set_tap_download(self, mask):
        """Which of the kept taps (TAP_DEBAYERED | TAP_COLOR) ``submit`` downloads into pinned memory with the result
        (rip_set_tap_download; default none): what a front end that publishes them on every frame wants."""
        self._call("rip_set_tap_download", int(mask))

    def _get_image(self, which, copy=True):
        """``copy=False``: for a frame that came through ``collect`` a read-only view of the handle's pinned host memory
        (rip_get_image_view; same lifetime as ``collect(copy=False)``); frames of ``process`` only exist on the device and are
        copied as before."""
        r, c, k = C.c_int(), C.c_int(), C.c_int()
        given = {IMAGE_DEBAYERED: self._given_last[1], IMAGE_COLOR: self._given_last[2], IMAGE_PROCESSED: self._given_last[0]}.get(which)
        if given is not None:  # the tap of the collected frame was downloaded into the caller's own array (submit(..., tap_*=))
            return given
        if not copy:
            view = C.c_void_p()
            self._call("rip_get_image_view", which, C.byref(view), C.byref(r), C.byref(c), C.byref(k))
            if view.value:
                n = r.value * c.value * k.value
                arr = np.frombuffer((C.c_uint8 * n).from_address(view.value), np.uint8)
                arr = arr.reshape((r.value, c.value) if k.value == 1 else (r.value, c.value, k.value))
                arr.flags.writeable = False
                return arr
        self._call("rip_get_image", which, None, C.c_size_t(0), C.byref(r), C.byref(c), C.byref(k))
        if r.value == 0 or c.value == 0:
            return np.empty((0, 0), np.uint8)
        shape = (r.value, c.value) if k.value == 1 else (r.value, c.value, k.value)
        out = self.out_pool.take(shape) if self.out_pool is not None else np.empty(shape, np.uint8)
        self._call("rip_get_image", which, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size), C.byref(r), C.byref(c),
                   C.byref(k))
        return out

    def get_dist_debayered_image(self, copy=True):
        return self._get_image(IMAGE_DEBAYERED, copy)

    def get_dist_color_image(self, copy=True):
        return self._get_image(IMAGE_COLOR, copy)

    def get_rect_mask(self):
        """The valid-pixel mask of the last frame's geometry, an (R, C) uint8 array of the maps' size, under ``set_rect_mask``
        "coverage" / "valid" after a frame that was undistorted; else empty, as the reference's never-written rect_mask_ is."""
        return self._get_image(IMAGE_RECT_MASK)

    def set_rect_mask(self, mode):
        """Extension: valid-pixel masks -- "off" (default), "coverage" (cv::remap of an all-255 image: 0 outside the source, 255
        inside, in between on the rim) or "valid" (255 where the coverage is 255, else 0).  The frame calls are not affected; the
        masks are built by ``get_rect_mask`` / ``get_output_mask`` and cached on the device.  include/rip.h rip_set_rect_mask."""
        self._call("rip_set_rect_mask", mode.encode())

    def get_rect_mask_mode(self):
        return self._string("rip_get_rect_mask_mode")

    def get_output_mask(self, rows, cols, channels, encoding):
        """The mask of the image the selected head delivers for such an input frame, (H, W) uint8: the head's window, size, fit mode
        and filter applied to the coverage (letterbox bands are 0), thresholded behind them under "valid".  No frame need have
        been processed.  include/rip.h rip_get_output_mask."""
        h, w = C.c_int(), C.c_int()
        geometry = (int(rows), int(cols), int(channels), encoding.encode())
        self._call("rip_get_output_mask", *geometry, None, C.c_size_t(0), C.byref(h), C.byref(w))
        out = np.empty((h.value, w.value), np.uint8)
        self._call("rip_get_output_mask", *geometry, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size), C.byref(h), C.byref(w))
        return out

    def get_output_mask_device(self, rows, cols, channels, encoding):
        """(device pointer, row pitch in bytes, H, W) of the same mask where the handle caches it: written in the order of the
        handle's stream, valid until that head's cache is dropped.  include/rip.h rip_get_output_mask_device."""
        ptr, pitch, h, w = C.c_void_p(), C.c_size_t(), C.c_int(), C.c_int()
        self._call("rip_get_output_mask_device", int(rows), int(cols), int(channels), encoding.encode(), C.byref(ptr), C.byref(pitch),
                   C.byref(h), C.byref(w))
        return ptr.value, pitch.value, h.value, w.value

    def debug_rect_mask_info(self, head):
        """(mask builds, head builds): test hook, include/rip.h rip_debug_rect_mask_info."""
        m, k = C.c_int(), C.c_int()
        self._call("rip_debug_rect_mask_info", int(head), C.byref(m), C.byref(k))
        return m.value, k.value

    def get_processed_image(self, copy=True):
        return self._get_image(IMAGE_PROCESSED, copy)

    # ---- loaders ---------------------------------------------------------------------------------
    def load_params(self, path):
        try:
            self._call("rip_load_params", path.encode())
        finally:
            self._output_format = self.get_output_format()  # the params file's `output: format:` (head 0 is selected after a load)

    def load_camera_calibration(self, path):
        self._call("rip_load_camera_calibration", path.encode())

    def load_color_calibration(self, path):
        self._call("rip_load_color_calibration", path.encode())

    def init_undistortion(self):
        self._call("rip_init_undistortion")

    def load_ccc_model(self, path):
        self._call("rip_load_ccc_model", path.encode())

    def set_ccc_model(self, filt, bias):
        filt = np.ascontiguousarray(filt, np.float32)
        bias = np.ascontiguousarray(bias, np.float32)
        if filt.shape != bias.shape or filt.ndim != 2:
            raise ValueError("filter and bias must be 2-D arrays of the same shape")
        self._call("rip_set_ccc_model", int(filt.shape[1]), int(filt.shape[0]), filt.ctypes.data_as(C.c_void_p),
                   bias.ctypes.data_as(C.c_void_p))

    def set_ccc_kalman_model(self, h, r):
        self._call("rip_set_ccc_kalman_model", C.c_double(h), C.c_double(r))

    # ---- other interfaces ------------------------------------------------------------------------
    def reset_white_balance_temporal_consistency(self):
        self._call("rip_reset_white_balance_temporal_consistency")

    def set_gpu(self, use_gpu):
        self._call("rip_set_gpu", int(bool(use_gpu)))

    def set_debug(self, debug):
        """While on, process()/apply() of an 8-bit frame also write the image after each of the eight modules to
        /tmp/0N_<module>.png (RIP_DEBUG_DIR replaces /tmp), min-max normalised like the reference's saveDebugImage
        (raw_image_pipeline.hpp:143-186)."""
        self._call("rip_set_debug", int(bool(debug)))

    def set_fp_contraction(self, mode):
        """Not in the reference: the floating-point contraction model of the float stages -- 0 (default) every product and
        sum rounded (OpenCV built for baseline x86-64), 1 the fused forms of an FMA-target build (aarch64 / Jetson).
        include/rip.h rip_set_fp_contraction."""
        self._call("rip_set_fp_contraction", int(mode))

    DEBUG_DUMP_NAMES = ("00_debayer", "01_flip", "02_white_balancing", "03_color_calibration", "04_gamma_correction",
                        "05_vignetting_correction", "06_color_enhancer", "07_undistortion")

    def debug_write_png(self, path, image, normalize=True):
        """Test hook: the PNG writer (and min-max normalisation) of the debug dumps on a host image (H x W or H x W x 3 BGR)."""
        a = np.ascontiguousarray(image, np.uint8)
        cn = 1 if a.ndim == 2 else a.shape[2]
        self._check(self._lib.rip_debug_write_png(self._h, str(path).encode(), a.ctypes.data_as(C.c_void_p), int(a.shape[0]),
                                                  int(a.shape[1]), int(cn), int(bool(normalize))))

    # ---- setters (names as in raw_image_pipeline_python.cpp:25-58) --------------------------------
    def set_debayer(self, enabled):
        self._call("rip_set_debayer", int(bool(enabled)))

    def set_debayer_16bit(self, enabled):
        """Extension: accept bayer_*16 frames instead of raising like the reference: debayer + flip only and bgr16 out, or --
        with ``set_debayer_16bit_range`` -- the whole pipeline and bgr8 out."""
        self._call("rip_set_debayer_16bit", int(bool(enabled)))

    def set_debayer_16bit_range(self, black, white):
        """Extension: black and white level of bayer_*16 frames; (0, 0) = off.  With ``set_debayer_16bit(True)`` and
        0 <= black < white <= 65535 such a frame is demosaiced at 16 bits, narrowed to 8 bits (255 (v - black) / (white - black),
        rounded half up, clamped) and then processed like a bgr8 frame: every stage, the taps, uint8 ``bgr8`` out.
        include/rip.h rip_set_debayer_16bit_range."""
        self._call("rip_set_debayer_16bit_range", int(black), int(white))

    def get_debayer_16bit_range(self):
        b, w = C.c_int(), C.c_int()
        self._call("rip_get_debayer_16bit_range", C.byref(b), C.byref(w))
        return b.value, w.value

    def set_debayer_encoding(self, encoding):
        self._call("rip_set_debayer_encoding", encoding.encode())

    def set_debayer_method(self, method):
        """Extension: "bilinear" (default, the reference's CPU path) or "mht" (Malvar-He-Cutler, what its CUDA path's
        cv::cuda::demosaicing(..., COLOR_Bayer**2BGR_MHT) computes).  include/rip.h rip_set_debayer_method."""
        self._call("rip_set_debayer_method", method.encode())

    def get_debayer_method(self):
        return self._string("rip_get_debayer_method")

    def set_output_format(self, name):
        """Extension: what the frame calls deliver -- "native" (default: the pipeline's own image, nothing added), "rgb8",
        "mono8", or the planar tensors "rgb_chw_f32" / "rgb_chw_f16" / "rgb_chw_bf16" / "bgr_chw_f32" / "bgr_chw_f16" /
        "bgr_chw_bf16" normalised by ``set_output_normalization``.  ``process`` / ``apply`` / ``collect`` then return uint8
        [R, C, 3] / [R, C] or float32 / float16 [3, R, C]; bf16 comes back as uint16 bit patterns [3, R, C] (numpy has no
        bfloat16; ``apply_device`` returns a torch.bfloat16 tensor).  include/rip.h rip_set_output_format."""
        self._call("rip_set_output_format", name.encode())
        self._output_format = name

    def get_output_format(self):
        return self._string("rip_get_output_format")

    def set_output_yuv_matrix(self, name):
        """Extension: the matrix and range of the formats "nv12" / "i420" -- "bt601" (default), "bt709", "bt601_full" or
        "bt709_full"; a setting of the selected output head, without effect under any other format.  The frame calls then deliver
        uint8 [3 H / 2, W] (``yuv_planes`` takes it apart).  include/rip.h rip_set_output_yuv_matrix."""
        self._call("rip_set_output_yuv_matrix", name.encode())

    def get_output_yuv_matrix(self):
        return self._string("rip_get_output_yuv_matrix")

    def set_output_normalization(self, divisor=255.0, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
        """Extension: the planar formats deliver ``(v / divisor - mean[c]) / std[c]`` for plane c (mean / std in the order of
        the format's planes), evaluated in double and rounded to the element type.  include/rip.h rip_set_output_normalization."""
        m, _ = _as_doubles(list(mean))
        s, _ = _as_doubles(list(std))
        if len(m) != 3 or len(s) != 3:
            raise ValueError("mean and std take 3 values")
        self._call("rip_set_output_normalization", C.c_double(divisor), m, s)

    def get_output_normalization(self):
        d, m, s = C.c_double(), (C.c_double * 3)(), (C.c_double * 3)()
        self._call("rip_get_output_normalization", C.byref(d), m, s)
        return d.value, tuple(m), tuple(s)

    def set_output_size(self, width, height):
        """Extension: resize the delivered frames to ``width`` x ``height`` on the GPU, in front of the output format --
        cv::resize(F, (width, height), INTER_LINEAR) on the pipeline's final 8-bit image, bit for bit.  (0, 0) (default) is off;
        a target equal to the image's own size changes nothing.  ``process`` / ``collect`` / ``apply_device`` then return arrays
        of the delivered height x width; the taps keep the pipeline's geometry.  include/rip.h rip_set_output_size."""
        self._call("rip_set_output_size", int(width), int(height))

    def get_output_size(self):
        w, h = C.c_int(), C.c_int()
        self._call("rip_get_output_size", C.byref(w), C.byref(h))
        return w.value, h.value

    def set_output_interpolation(self, name):
        """Extension: the filter of the resize stage, ``"linear"`` (default), ``"area"`` -- cv::resize's INTER_AREA for
        downscales, which averages every source pixel an output pixel covers -- or ``"linear_aa"`` / ``"cubic_aa"``: byte for byte
        ``torch.nn.functional.interpolate(uint8, mode='bilinear' / 'bicubic', antialias=True)``, which is what
        ``torchvision.transforms.v2.Resize`` computes on uint8 tensors, for downscales and upscales.  Without effect until
        ``set_output_size`` has set a target; under ``"area"`` a target larger than the image, or more than 256 times smaller, on an
        axis is refused by the frame calls (ValueError), under the two antialiased names a target more than 64 times smaller.
        include/rip.h rip_set_output_interpolation."""
        self._call("rip_set_output_interpolation", name.encode())

    def get_output_interpolation(self):
        return self._string("rip_get_output_interpolation")

    def set_output_roi(self, x, y, width, height):
        """Extension: the window (x, y, width, height) of the pipeline's final image that the resize stage reads in place of the whole
        image; (0, 0, 0, 0) (default) is off.  Without a target size the frame calls deliver the window itself.  A window that does
        not lie inside the image is refused by the frame calls and the queries (ValueError).  include/rip.h rip_set_output_roi."""
        self._call("rip_set_output_roi", int(x), int(y), int(width), int(height))

    def get_output_roi(self):
        v = [C.c_int() for _ in range(4)]
        self._call("rip_get_output_roi", *[C.byref(i) for i in v])
        return tuple(i.value for i in v)

    def set_output_fit(self, name):
        """Extension: how the window is placed in the target size -- ``"stretch"`` (default), ``"letterbox"`` (aspect kept, the
        rest padded) or ``"crop"`` (the centred part with the target's aspect).  Without effect until ``set_output_size`` has set
        a target.  include/rip.h rip_set_output_fit."""
        self._call("rip_set_output_fit", name.encode())

    def get_output_fit(self):
        return self._string("rip_get_output_fit")

    def set_output_pad(self, b, g, r):
        """Extension: the colour (B, G, R of the image in front of the output format, each 0..255, default 114) of what a
        letterbox leaves uncovered.  include/rip.h rip_set_output_pad."""
        self._call("rip_set_output_pad", int(b), int(g), int(r))

    def get_output_pad(self):
        v = [C.c_int() for _ in range(3)]
        self._call("rip_get_output_pad", *[C.byref(i) for i in v])
        return tuple(i.value for i in v)

    def set_output_clahe(self, clip_limit, tiles_x, tiles_y):
        """Extension: CLAHE, ``cv2.createCLAHE(clip_limit, (tiles_x, tiles_y)).apply`` restated, on the delivered one-channel picture
        of the selected output head (a mono camera, or the format "mono8"); the last launch of the head, letterbox bands stay as they
        are.  clip_limit >= 0 (0: no clipping), tiles both in 1..16 or (0, 0) for off.  include/rip.h rip_set_output_clahe."""
        self._call("rip_set_output_clahe", C.c_double(clip_limit), int(tiles_x), int(tiles_y))

    def set_output_jpeg(self, quality=90, restart_rows=1):
        """Extension: the quality (1..100, the IJG scaling of the Annex K tables) and the MCU rows per restart interval (1..64) of the
        output format "jpeg" of the selected output head; without effect under any other format.  include/rip.h rip_set_output_jpeg."""
        self._call("rip_set_output_jpeg", int(quality), int(restart_rows))

    def get_output_jpeg(self):
        """(quality, restart_rows) of the selected output head."""
        q, r = C.c_int(), C.c_int()
        self._call("rip_get_output_jpeg", C.byref(q), C.byref(r))
        return q.value, r.value

    def jpeg_sizes(self, head=None):
        """The stream lengths (numpy uint32 [n]) of the frames of the last frame call of the selected output head (or ``head``): empty
        when that call delivered another format; an entry 0: the stream did not fit its slot, which was left untouched.  Waits for
        the handle's stream (rip_get_output_jpeg_sizes)."""
        was = None
        if head is not None and int(head) != self.get_selected_output_head():
            was = self.get_selected_output_head()
            self._call("rip_select_output_head", int(head))
        try:
            n = C.c_int()
            self._call("rip_get_output_jpeg_sizes", None, 0, C.byref(n))
            sizes = np.zeros(n.value, np.uint32)
            if n.value:
                self._call("rip_get_output_jpeg_sizes", sizes.ctypes.data_as(C.c_void_p), n.value, C.byref(n))
            return sizes
        finally:
            if was is not None:
                self._call("rip_select_output_head", was)

    def get_output_clahe(self):
        """(clip_limit, tiles_x, tiles_y) of the selected output head."""
        clip, tx, ty = C.c_double(), C.c_int(), C.c_int()
        self._call("rip_get_output_clahe", C.byref(clip), C.byref(tx), C.byref(ty))
        return clip.value, tx.value, ty.value

    def get_output_window(self, rows, cols, channels, encoding):
        """((x, y, w, h) of the final image that is read, (x, y, w, h) of the delivered image that holds picture) for such an input
        frame; everything outside the second rectangle is pad.  include/rip.h rip_get_output_window."""
        src, dst = (C.c_int * 4)(), (C.c_int * 4)()
        self._call("rip_get_output_window", int(rows), int(cols), int(channels), encoding.encode(), src, dst)
        return tuple(src), tuple(dst)

    def get_output_camera_info(self, rows, cols, channels, encoding):
        """(height, width, K [3, 3], P [3, 4]) of the image the frame calls deliver for such an input frame: the rect (or, without
        undistortion, dist) matrices scaled to the target size about the pixel centres.  include/rip.h rip_get_output_camera_info."""
        h, w = C.c_int(), C.c_int()
        k, pr = (C.c_double * 9)(), (C.c_double * 12)()
        self._call("rip_get_output_camera_info", int(rows), int(cols), int(channels), encoding.encode(), C.byref(h), C.byref(w), k, pr)
        return h.value, w.value, np.array(k, dtype=np.float64).reshape(3, 3), np.array(pr, dtype=np.float64).reshape(3, 4)

    def set_flip(self, enabled):
        self._call("rip_set_flip", int(bool(enabled)))

    def set_flip_angle(self, angle):
        self._call("rip_set_flip_angle", int(angle))

    def set_white_balance(self, enabled):
        self._call("rip_set_white_balance", int(bool(enabled)))

    def set_white_balance_method(self, method):
        self._call("rip_set_white_balance_method", method.encode())

    def set_white_balance_percentile(self, percentile):
        self._call("rip_set_white_balance_percentile", C.c_double(percentile))

    def set_white_balance_saturation_threshold(self, bright_thr, dark_thr):
        self._call("rip_set_white_balance_saturation_threshold", C.c_double(bright_thr), C.c_double(dark_thr))

    def set_white_balance_temporal_consistency(self, enabled):
        self._call("rip_set_white_balance_temporal_consistency", int(bool(enabled)))

    def set_gamma_correction(self, enabled):
        self._call("rip_set_gamma_correction", int(bool(enabled)))

    def set_gamma_correction_method(self, method):
        self._call("rip_set_gamma_correction_method", method.encode())

    def set_gamma_correction_k(self, k):
        self._call("rip_set_gamma_correction_k", C.c_double(k))

    def set_vignetting_correction(self, enabled):
        self._call("rip_set_vignetting_correction", int(bool(enabled)))

    def set_vignetting_correction_parameters(self, scale, a2, a4):
        self._call("rip_set_vignetting_correction_parameters", C.c_double(scale), C.c_double(a2), C.c_double(a4))

    def set_color_enhancer(self, enabled):
        self._call("rip_set_color_enhancer", int(bool(enabled)))

    def set_color_enhancer_hue_gain(self, gain):
        self._call("rip_set_color_enhancer_hue_gain", C.c_double(gain))

    def set_color_enhancer_saturation_gain(self, gain):
        self._call("rip_set_color_enhancer_saturation_gain", C.c_double(gain))

    def set_color_enhancer_value_gain(self, gain):
        self._call("rip_set_color_enhancer_value_gain", C.c_double(gain))

    def set_color_calibration(self, enabled):
        self._call("rip_set_color_calibration", int(bool(enabled)))

    def set_color_calibration_matrix(self, matrix):
        arr, n = _as_doubles(list(np.asarray(matrix, dtype=np.float64).reshape(-1)))
        self._call("rip_set_color_calibration_matrix", arr, n)

    def set_color_calibration_bias(self, bias):
        arr, n = _as_doubles(list(np.asarray(bias, dtype=np.float64).reshape(-1)))
        self._call("rip_set_color_calibration_bias", arr, n)

    def set_undistortion(self, enabled):
        self._call("rip_set_undistortion", int(bool(enabled)))

    def set_undistortion_image_size(self, width, height):
        self._call("rip_set_undistortion_image_size", int(width), int(height))

    def set_undistortion_new_image_size(self, width, height):
        self._call("rip_set_undistortion_new_image_size", int(width), int(height))

    def set_undistortion_balance(self, balance):
        self._call("rip_set_undistortion_balance", C.c_double(balance))

    def set_undistortion_fov_scale(self, fov_scale):
        self._call("rip_set_undistortion_fov_scale", C.c_double(fov_scale))

    def _set_vec(self, name, values):
        arr, n = _as_doubles(list(np.asarray(values, dtype=np.float64).reshape(-1)))
        self._call(name, arr, n)

    def set_undistortion_camera_matrix(self, m):
        self._set_vec("rip_set_undistortion_camera_matrix", m)

    def set_undistortion_distortion_coeffs(self, d):
        """All values given are passed on: 4 for the fisheye models, 5 for plumb_bob, 8 for rational_polynomial."""
        self._set_vec("rip_set_undistortion_distortion_coefficients", d)

    set_undistortion_distortion_coefficients = set_undistortion_distortion_coeffs

    def set_undistortion_distortion_model(self, model):
        self._call("rip_set_undistortion_distortion_model", model.encode())

    def set_undistortion_rectification_matrix(self, m):
        self._set_vec("rip_set_undistortion_rectification_matrix", m)

    def set_undistortion_projection_matrix(self, m):
        self._set_vec("rip_set_undistortion_projection_matrix", m)

    # ---- getters -----------------------------------------------------------------------------------
    def _flag(self, name):
        return bool(getattr(self._lib, name)(self._h))

    def is_debayer_enabled(self):
        return self._flag("rip_is_debayer_enabled")

    def is_flip_enabled(self):
        return self._flag("rip_is_flip_enabled")

    def is_white_balance_enabled(self):
        return self._flag("rip_is_white_balance_enabled")

    def is_color_calibration_enabled(self):
        return self._flag("rip_is_color_calibration_enabled")

    def is_gamma_correction_enabled(self):
        return self._flag("rip_is_gamma_correction_enabled")

    def is_vignetting_correction_enabled(self):
        return self._flag("rip_is_vignetting_correction_enabled")

    def is_color_enhancer_enabled(self):
        return self._flag("rip_is_color_enhancer_enabled")

    def is_undistortion_enabled(self):
        return self._flag("rip_is_undistortion_enabled")

    def get_dist_image_height(self):
        return int(self._lib.rip_get_dist_image_height(self._h))

    def get_dist_image_width(self):
        return int(self._lib.rip_get_dist_image_width(self._h))

    def get_rect_image_height(self):
        return int(self._lib.rip_get_rect_image_height(self._h))

    def get_rect_image_width(self):
        return int(self._lib.rip_get_rect_image_width(self._h))

    def _string(self, name):
        buf = C.create_string_buffer(64)
        self._call(name, buf, C.c_size_t(64))
        return buf.value.decode(errors="replace")

    def get_dist_distortion_model(self):
        return self._string("rip_get_dist_distortion_model")

    def get_rect_distortion_model(self):
        return self._string("rip_get_rect_distortion_model")

    def _matrix(self, name, shape):
        n = int(np.prod(shape))
        buf = (C.c_double * n)()
        self._call(name, buf)
        return np.array(buf, dtype=np.float64).reshape(shape)

    def get_color_calibration_matrix(self):
        return self._matrix("rip_get_color_calibration_matrix", (3, 3))

    def get_color_calibration_bias(self):
        return self._matrix("rip_get_color_calibration_bias", (4, 1))

    def get_dist_camera_matrix(self):
        return self._matrix("rip_get_dist_camera_matrix", (3, 3))

    def _coefficients(self, rect):
        # 1 x n: n = 5 for plumb_bob and radtan, 8 for rational_polynomial, 4 for every other model (include/rip.h)
        buf, n = (C.c_double * 8)(), C.c_int()
        self._call("rip_get_distortion_coefficients_n", int(rect), buf, 8, C.byref(n))
        return np.array(buf[:n.value], dtype=np.float64).reshape(1, n.value)

    def get_dist_distortion_coefficients(self):
        return self._coefficients(0)

    def get_dist_rectification_matrix(self):
        return self._matrix("rip_get_dist_rectification_matrix", (3, 3))

    def get_dist_projection_matrix(self):
        return self._matrix("rip_get_dist_projection_matrix", (3, 4))

    def get_rect_camera_matrix(self):
        return self._matrix("rip_get_rect_camera_matrix", (3, 3))

    def get_rect_distortion_coefficients(self):
        return self._coefficients(1)

    def get_rect_rectification_matrix(self):
        return self._matrix("rip_get_rect_rectification_matrix", (3, 3))

    def get_rect_projection_matrix(self):
        return self._matrix("rip_get_rect_projection_matrix", (3, 4))

    # ---- introspection ------------------------------------------------------------------------------
    def get_undistortion_maps(self):
        r, c = C.c_int(), C.c_int()
        self._call("rip_get_undistortion_maps", None, None, C.c_size_t(0), C.byref(r), C.byref(c))
        mx = np.empty((r.value, c.value), np.float32)
        my = np.empty((r.value, c.value), np.float32)
        self._call("rip_get_undistortion_maps", mx.ctypes.data_as(C.c_void_p), my.ctypes.data_as(C.c_void_p),
                   C.c_size_t(mx.size), C.byref(r), C.byref(c))
        return mx, my

    def get_white_balance_info(self, n_frames=1):
        buf = np.empty((n_frames, 8), np.float32)
        self._call("rip_get_white_balance_info", buf.ctypes.data_as(C.c_void_p), int(n_frames))
        return buf

    def get_ccc_track(self, n_frames=1):
        """(n, 4) int32: raw argmax (x, y) and filtered (x, y) of the ccc estimator for the frames of the last batch."""
        buf = np.empty((n_frames, 4), np.int32)
        self._call("rip_get_ccc_track", buf.ctypes.data_as(C.c_void_p), int(n_frames))
        return buf

    def debug_plan_info(self, src_rows, src_cols):
        """Test hook (rip_debug_plan_info): dict describing the compiled remap plan of the current calibration."""
        info = (C.c_int * 9)()
        self._call("rip_debug_plan_info", int(src_rows), int(src_cols), info)
        keys = ("tiles_x", "tiles_y", "border_pixels", "max_lds_bytes", "max_rect_w", "max_rect_h", "on_device", "tile_w", "tile_h")
        return dict(zip(keys, [int(v) for v in info]))

    def debug_chain_footprint(self, src_rows, src_cols, flip_angle=0):
        """Test hook (rip_debug_chain_footprint): (dict, intervals) -- the items the fused chain walks in front of the remap
        and, per row pair of the chain's input, the walked groups [lo, hi) as an (src_rows // 2, 2) int32 array."""
        info = (C.c_int * 4)()
        iv = np.zeros((int(src_rows) // 2, 2), np.int32)
        self._call("rip_debug_chain_footprint", int(src_rows), int(src_cols), int(flip_angle), info, iv.ctypes.data_as(C.c_void_p),
                   int(iv.shape[0]))
        keys = ("dense_items", "footprint_items", "row_pairs", "last_walked")
        return dict(zip(keys, [int(v) for v in info])), iv

    def launch_log(self):
        """Test hook (rip_debug_launch_log): ``with pipe.launch_log() as log:`` records every kernel launch the handle's
        calls make inside the block; afterwards ``log.records()`` gives them as dicts and ``log.names()`` as the kernels'
        names with their template arguments, e.g. ``chain_fast_kernel<7, 1, 512, false>``."""
        return LaunchLog(self)

    def _launch_log_text(self):
        need = C.c_size_t(0)
        self._lib.rip_debug_get_launch_log(self._h, None, C.c_size_t(0), C.byref(need))
        buf = C.create_string_buffer(max(1, need.value))
        self._call("rip_debug_get_launch_log", buf, C.c_size_t(len(buf)), C.byref(need))
        return buf.value.decode()

    def set_tunable(self, name, value):
        """Launch tunable of this handle (rip_set_tunable: development / test hook; the library reads its environment
        overrides once, when the handle is created)."""
        self._call("rip_set_tunable", name.encode(), int(value))

    PROBE_KINDS = {"copy": 0, "read": 1, "fill": 2, "expand13": 3, "expand13_nt": 4, "copy12": 5, "expand13_wide": 6, "expand13_wide_nt": 7, "read_nt": 8, "expand13_coalesced": 9, "expand13_coalesced_nt": 10}

    def hbm_probe(self, kind, nbytes=1 << 30, reps=10):
        """GB/s (best of ``reps`` launches, bytes read + written) of one of the library's hand-written streaming kernels on
        this handle's device and stream (rip_debug_hbm_probe): the measured ceiling a kernel of that access shape can reach
        on this box."""
        out = C.c_double()
        self._call("rip_debug_hbm_probe", int(self.PROBE_KINDS.get(kind, kind)), C.c_size_t(int(nbytes)), int(reps), C.byref(out))
        return out.value

    KERNEL_CLASSES = ("stats", "ccc", "chain", "remap")

    def profile_begin(self, max_records):
        self._call("rip_profile_begin", int(max_records))

    def profile_end(self):
        """-> {class: (total_ms, launches)} from HIP events on the handle's stream."""
        ms = (C.c_double * 4)()
        cnt = (C.c_int * 4)()
        self._call("rip_profile_end", ms, cnt)
        return {k: (ms[i], cnt[i]) for i, k in enumerate(self.KERNEL_CLASSES)}

    def debug_atan(self, values):
        """atan of the device map builder (double-double, rip_maps.hip) for an array of doubles."""
        a = np.ascontiguousarray(values, np.float64)
        out = np.empty_like(a)
        self._check(self._lib.rip_debug_atan(self._h, a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), int(a.size)))
        return out

    def get_vignetting_mask(self, rows, cols):
        """Host-built mask plane of precomputeVignettingMask (vignetting_correction.cpp:32-63)."""
        out = np.empty((int(rows), int(cols)), np.float32)
        self._check(self._lib.rip_get_vignetting_mask(self._h, int(rows), int(cols), out.ctypes.data_as(C.c_void_p),
                                                      C.c_size_t(out.size)))
        return out

    def get_table(self, which):
        buf = np.empty(4096, np.int32)
        n = self._lib.rip_get_table(self._h, int(which), buf.ctypes.data_as(C.c_void_p), 4096)
        if n < 0:
            raise ValueError("unknown table id")
        return buf[:n].copy()
