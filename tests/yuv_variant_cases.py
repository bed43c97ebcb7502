"""One case per kernel of the library librip_yuv_hip.so (csrc/rip_yuv.hip): which output format makes exactly that kernel run behind the
pipeline's image.  tests/test_yuv_variants.py (CPU) checks that the table is exactly the library's kernels -- in both directions;
tests/test_yuv_gpu.py runs the case and reads the handle's launch log.

Importable without a GPU; nothing here looks at the library."""
import collections

Case = collections.namedtuple("Case", ["name", "fc", "format"])

CASES = [
    Case("yuv420_kernel<true>", 0, "nv12"),      # semi-planar: interleaved chroma rows
    Case("yuv420_kernel<false>", 0, "i420"),     # two chroma planes
]
TABLE = {(c.name, c.fc): c for c in CASES}
assert len(TABLE) == len(CASES), "two cases for one record"


def case_id(case):
    return case.name
