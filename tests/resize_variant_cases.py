"""One case per kernel instantiation of the companion library librip_rsz_hip.so (csrc/rip_resize.hip): which input encoding and
which pair of sizes make exactly that resize kernel run.  tests/test_resize_variants.py (CPU) checks that the table is exactly
the companion's instantiations -- in both directions; tests/test_resize_gpu.py runs every case, reads the handle's launch log and
compares the delivered frames with oracle.resize_linear.

Importable without a GPU; nothing here looks at the library.

Sizes (w, h): the linear cases go from 1747 x 9 to 1027 x 5 -- two workgroups of 1024 pixels per row, the second one ragged with
a last lane of 3 pixels, a non-integer scale of about 1.7 on both axes; the 2 x 2 cases halve 2050 x 10 to 1025 x 5 (a last lane
of 1 pixel)."""
import collections

Case = collections.namedtuple("Case", ["name", "fc", "encoding", "channels", "src_size", "dst_size", "n_frames"])

CASES = [
    Case("resize_kernel<1, false>", 0, "mono8", 1, (1747, 9), (1027, 5), 3),
    Case("resize_kernel<3, false>", 0, "bgr8", 3, (1747, 9), (1027, 5), 3),
    Case("resize_kernel<1, true>", 0, "mono8", 1, (2050, 10), (1025, 5), 3),
    Case("resize_kernel<3, true>", 0, "bgr8", 3, (2050, 10), (1025, 5), 3),
]
TABLE = {(c.name, c.fc): c for c in CASES}
assert len(TABLE) == len(CASES), "two cases for one record"


def kernel_name(channels, area2):
    return "resize_kernel<%d, %s>" % (channels, "true" if area2 else "false")


def case_id(case):
    return case.name
