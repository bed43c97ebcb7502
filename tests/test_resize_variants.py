"""The table of tests/resize_variant_cases.py is closed over the companion library librip_rsz_hip.so: every instantiation of the
resize kernel has a case and every case names a kernel that exists; the two other libraries hold no resize kernel.  Reads the
symbol tables (the host-side launch stubs) with the parser of tests/test_variant_cases.py; no instruction stream."""
import os

import resize_variant_cases as RV
from test_variant_cases import instantiations


def rsz_path():
    from raw_image_pipeline_amd import build as B
    return B.OUT_RSZ


def test_the_companion_is_built_next_to_the_library(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    assert os.path.exists(rsz_path())
    assert os.path.dirname(rsz_path()) == os.path.dirname(LIB_PATH)
    assert hasattr(rip_lib, "rip_set_output_size")


def test_the_table_is_exactly_the_companions_instantiations(rip_lib):
    names = instantiations(rsz_path())
    assert all(count == 1 for count in names.values()), names
    records = {(name, 0) for name in names}
    table = set(RV.TABLE)
    missing = sorted(records - table)
    assert not missing, "instantiations without a case (tests/resize_variant_cases.py): %s" % missing
    stale = sorted(table - records)
    assert not stale, "entries name kernels the companion does not hold: %s" % stale
    assert len(RV.CASES) == 4
    assert {c.name for c in RV.CASES} == {RV.kernel_name(ch, a) for ch in (1, 3) for a in (False, True)}


def test_the_other_libraries_hold_no_resize_kernel(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    for so in (LIB_PATH, B.OUT_COMPANION):
        assert not [n for n in instantiations(so) if "resize_kernel" in n], so


def test_up_to_date_covers_the_companion(rip_lib):
    from raw_image_pipeline_amd import build as B
    assert B.up_to_date() and B.rsz_up_to_date()
    for f in B.RSZ_SOURCES + B.RSZ_HEADERS:
        assert os.path.exists(os.path.join(B.CSRC, f))
    assert "rip_resize.hpp" in B.HEADERS     # rip_handle.hpp includes it: librip_hip.so is rebuilt when the interface changes
