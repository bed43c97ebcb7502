"""One case per kernel instantiation of the companion library librip_aa_hip.so (csrc/rip_aa.hip): which input encoding, which window
and which pair of sizes make exactly that kernel run under rip_set_output_interpolation("linear_aa" / "cubic_aa").
tests/test_aa_variants.py (CPU) checks that the table is exactly the companion's instantiations -- in both directions;
tests/test_resize_aa_gpu.py runs every case, reads the handle's launch log and compares the delivered frames with
tests/aa_reference.py.

Importable without a GPU; nothing here looks at the library.

Sizes (w, h): from 200 x 29 (or a window of that size at (3, 2) of a 210 x 33 image, the first byte of a row of the window at phase
1 under three channels and 3 under one) to 133 x 19 -- three workgroups of 64 columns, three of 8 rows, the last ones ragged."""
import collections

Case = collections.namedtuple("Case", ["name", "fc", "encoding", "channels", "frame_size", "roi", "dst_size", "n_frames", "filter"])

CASES = [
    Case("aa_kernel<1, false>", 0, "mono8", 1, (200, 29), None, (133, 19), 3, "linear_aa"),
    Case("aa_kernel<3, false>", 0, "bgr8", 3, (200, 29), None, (133, 19), 3, "cubic_aa"),
    Case("aa_kernel<1, true>", 0, "mono8", 1, (210, 33), (3, 2, 200, 29), (133, 19), 3, "cubic_aa"),
    Case("aa_kernel<3, true>", 0, "bgr8", 3, (210, 33), (3, 2, 200, 29), (133, 19), 3, "linear_aa"),
]
TABLE = {(c.name, c.fc): c for c in CASES}
assert len(TABLE) == len(CASES), "two cases for one record"


def kernel_name(channels, window):
    return "aa_kernel<%d, %s>" % (channels, "true" if window else "false")


def case_id(case):
    return case.name
