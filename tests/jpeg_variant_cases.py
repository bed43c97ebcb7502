"""One case per kernel of the library librip_jpeg_hip.so (csrc/rip_jpeg.hip): every head that delivers "jpeg" launches four of them
per batch slice -- the transform of its channel count, then the sizing pass, the scan and the writing pass.  tests/test_jpeg_library.py
(CPU) checks that the table is exactly the library's kernels -- in both directions; tests/test_jpeg_gpu.py reads the handle's launch log.

Importable without a GPU; nothing here looks at the library."""
import collections

Case = collections.namedtuple("Case", ["name", "fc", "what"])

CASES = [
    Case("jpeg_transform_kernel<true>", 0, "B, G, R -> Y Cb Cr 4:2:0 blocks: forward DCT, quantiser, zigzag; one block per lane"),
    Case("jpeg_transform_kernel<false>", 0, "one channel -> blocks"),
    Case("jpeg_size_kernel", 0, "the stuffed byte count of every restart interval"),
    Case("jpeg_scan_kernel", 0, "offsets, stream lengths and the overflow decision per frame"),
    Case("jpeg_write_kernel", 0, "the bytes of every interval at their final position, the header and EOI"),
]
TABLE = {(c.name, c.fc): c for c in CASES}
assert len(TABLE) == len(CASES), "two cases for one record"


def launch_order(channels):
    return ["jpeg_transform_kernel<%s>" % ("true" if channels == 3 else "false"), "jpeg_size_kernel", "jpeg_scan_kernel", "jpeg_write_kernel"]


def case_id(case):
    return case.name
