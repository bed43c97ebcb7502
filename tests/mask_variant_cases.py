"""One case per kernel of the library librip_mask_hip.so (csrc/rip_mask.hip): which mode and which head make exactly that kernel run
through rip_get_output_mask.  tests/test_mask_variants.py (CPU) checks that the table is exactly the library's kernels -- in both
directions; tests/test_rect_mask_gpu.py runs the case and reads the handle's launch log.

Importable without a GPU; nothing here looks at the library."""
import collections

import heads_cases as HC

# mode: rip_set_rect_mask; head: the settings of the selected head on the undistorted 200 x 136 frame of tests/heads_cases.py
Case = collections.namedtuple("Case", ["name", "fc", "mode", "head"])

FRAME = "und200"
CASES = [
    # an identity head under "coverage" delivers M itself
    Case("rect_mask_kernel<false>", 0, "coverage", HC.IDENTITY),
    # ... and under "valid" the thresholded twin, which the kernel writes directly
    Case("rect_mask_kernel<true>", 0, "valid", HC.IDENTITY),
    # a head with a resize filters the coverage; "valid" thresholds behind it
    Case("mask_threshold_kernel", 0, "valid", HC.UPSCALE),
]
TABLE = {(c.name, c.fc): c for c in CASES}
assert len(TABLE) == len(CASES), "two cases for one record"


def case_id(case):
    return case.name
