"""One case per kernel of the library librip_heads_hip.so (csrc/rip_heads.hip): which head set of tests/heads_cases.py makes exactly
that kernel run through rip_apply_device_heads.  tests/test_heads_variants.py (CPU) checks that the table is exactly the library's
kernels -- in both directions; tests/test_heads_gpu.py runs the case and reads the handle's launch log.

Importable without a GPU; nothing here looks at the library."""
import collections

Case = collections.namedtuple("Case", ["name", "fc", "head_set", "copied_heads"])

CASES = [
    # the tight identity head of a 200 x 136 frame (600 bytes per row: no multiple of 16) is copied from the staging image
    Case("head_copy_kernel", 0, "mean_upscale_aa", (0,)),
]
TABLE = {(c.name, c.fc): c for c in CASES}
assert len(TABLE) == len(CASES), "two cases for one record"


def case_id(case):
    return case.name
