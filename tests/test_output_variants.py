"""The table of tests/output_variant_cases.py is closed over the companion library librip_out_hip.so: every instantiation of
the output stage's kernel has a case and every case names a kernel that exists; librip_hip.so itself has gained no kernel.
Reads the symbol tables (the host-side launch stubs) with the parser of tests/test_variant_cases.py; no instruction stream."""
import os

import output_variant_cases as OV
import variant_cases as V
from test_variant_cases import instantiations


def companion_path():
    from raw_image_pipeline_amd import build as B
    return B.OUT_COMPANION


def test_the_companion_is_built_next_to_the_library(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    assert os.path.exists(companion_path())
    assert os.path.dirname(companion_path()) == os.path.dirname(LIB_PATH)
    assert hasattr(rip_lib, "rip_set_output_format")


def test_the_table_is_exactly_the_companions_instantiations(rip_lib):
    names = instantiations(companion_path())
    assert all(count == 1 for count in names.values()), names
    records = {(name, 0) for name in names}
    table = set(OV.TABLE)
    missing = sorted(records - table)
    assert not missing, "instantiations without a case (tests/output_variant_cases.py): %s" % missing
    stale = sorted(table - records)
    assert not stale, "entries name kernels the companion does not hold: %s" % stale
    assert len(OV.CASES) == 8 and {c.format for c in OV.CASES} == {f for f, _ in OV.FORMAT_TAGS}


def test_the_core_library_has_gained_no_kernel(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    names = instantiations(LIB_PATH)
    assert not [n for n in names if "output_convert" in n]
    records = set()
    for name, count in names.items():
        records.add((name, 0))
        if count == 2:
            records.add((name, 1))
    assert len(records) == len(V.TABLE) + len(V.NOT_PRODUCT) + len(V.UNREACHABLE)


def test_up_to_date_covers_the_companion(rip_lib):
    from raw_image_pipeline_amd import build as B
    assert B.up_to_date() and B.companion_up_to_date()
    for f in B.COMPANION_SOURCES + B.COMPANION_HEADERS:
        assert os.path.exists(os.path.join(B.CSRC, f))
    assert "rip_output.hpp" in B.HEADERS     # rip_handle.hpp includes it: librip_hip.so is rebuilt when the interface changes
