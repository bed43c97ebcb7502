"""One case per kernel instantiation of the companion library librip_area_hip.so (csrc/rip_area.hip): which input encoding and which
pair of sizes make exactly that kernel run under rip_set_output_interpolation("area").  tests/test_area_variants.py (CPU) checks
that the table is exactly the companion's instantiations -- in both directions; tests/test_resize_area_gpu.py runs every case, reads
the handle's launch log and compares the delivered frames with tests/area_reference.py.

Importable without a GPU; nothing here looks at the library.

Sizes (w, h): the general cases go from 200 x 29 to 133 x 19 -- three workgroups of 64 x 8 pixels per axis, the last one ragged, a
factor of about 1.5; the whole-factor cases go from 201 x 27 to 67 x 9 (3 x 3 blocks, a second workgroup of 3 columns and 1 row)."""
import collections

Case = collections.namedtuple("Case", ["name", "fc", "encoding", "channels", "src_size", "dst_size", "n_frames"])

CASES = [
    Case("area_reduce_kernel<1, false>", 0, "mono8", 1, (200, 29), (133, 19), 3),
    Case("area_reduce_kernel<3, false>", 0, "bgr8", 3, (200, 29), (133, 19), 3),
    Case("area_reduce_kernel<1, true>", 0, "mono8", 1, (201, 27), (67, 9), 3),
    Case("area_reduce_kernel<3, true>", 0, "bgr8", 3, (201, 27), (67, 9), 3),
]
TABLE = {(c.name, c.fc): c for c in CASES}
assert len(TABLE) == len(CASES), "two cases for one record"


def kernel_name(channels, whole):
    return "area_reduce_kernel<%d, %s>" % (channels, "true" if whole else "false")


def case_id(case):
    return case.name
