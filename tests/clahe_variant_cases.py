"""One case per kernel of the library librip_clahe_hip.so (csrc/rip_clahe.hip): every head with CLAHE on launches both, the table
kernel and then the blend.  tests/test_clahe_library.py (CPU) checks that the table is exactly the library's kernels -- in both
directions; tests/test_clahe_gpu.py reads the handle's launch log.

Importable without a GPU; nothing here looks at the library."""
import collections

Case = collections.namedtuple("Case", ["name", "fc", "what"])

CASES = [
    Case("clahe_lut_kernel", 0, "one 256-byte table per (tile, frame)"),
    Case("clahe_apply_kernel", 0, "the blend of four tables per pixel"),
]
TABLE = {(c.name, c.fc): c for c in CASES}
assert len(TABLE) == len(CASES), "two cases for one record"
LAUNCH_ORDER = [c.name for c in CASES]


def case_id(case):
    return case.name
