"""The table of tests/heads_variant_cases.py is closed over the library librip_heads_hip.so: its one kernel has a case and the case
names a kernel that exists; no other library holds a head_copy_kernel and this one holds none of theirs.  Reads the symbol tables (the
host-side launch stubs) with the parser of tests/test_variant_cases.py; no instruction stream."""
import os

import heads_cases as HC
import heads_variant_cases as HV
from test_variant_cases import instantiations


def others():
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    return (LIB_PATH, B.OUT_COMPANION, B.OUT_RSZ, B.OUT_AREA, B.OUT_FIT, B.OUT_AA)


def test_the_library_is_built_next_to_the_others(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    assert os.path.basename(B.OUT_HEADS) == "librip_heads_hip.so" and os.path.exists(B.OUT_HEADS)
    assert os.path.dirname(B.OUT_HEADS) == os.path.dirname(LIB_PATH)
    assert hasattr(rip_lib, "rip_apply_device_heads") and hasattr(rip_lib, "rip_debug_output_head_info")


def test_the_table_is_exactly_the_librarys_kernels(rip_lib):
    from raw_image_pipeline_amd import build as B
    names = instantiations(B.OUT_HEADS)
    assert all(count == 1 for count in names.values()), names
    records = {(name, 0) for name in names}
    table = set(HV.TABLE)
    assert not sorted(records - table), "kernels without a case (tests/heads_variant_cases.py): %s" % sorted(records - table)
    assert not sorted(table - records), "entries name kernels the library does not hold: %s" % sorted(table - records)
    assert set(names) == {"head_copy_kernel"}
    for c in HV.CASES:
        heads = HC.BY_NAME[c.head_set].heads
        assert all(heads[k] == HC.IDENTITY for k in c.copied_heads)


def test_no_library_holds_a_kernel_of_another(rip_lib):
    from raw_image_pipeline_amd import build as B
    mine = set(instantiations(B.OUT_HEADS))
    for so in others():
        theirs = set(instantiations(so))
        assert not [n for n in theirs if "head_copy_kernel" in n], so
        assert not (mine & theirs), so
