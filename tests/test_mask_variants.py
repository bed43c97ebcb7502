"""The table of tests/mask_variant_cases.py is closed over the library librip_mask_hip.so: every kernel has a case and every case names
a kernel that exists, once each; no other library holds a rect_mask or mask_threshold kernel and this one holds none of theirs.  Reads
the symbol tables (the host-side launch stubs) with the parser of tests/test_variant_cases.py; no instruction stream.  And the build:
the third table of raw_image_pipeline_amd/build.py, its dating and the link."""
import os
import subprocess

import mask_variant_cases as MV
from test_variant_cases import instantiations


def others():
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    return (LIB_PATH, B.OUT_COMPANION, B.OUT_RSZ, B.OUT_AREA, B.OUT_FIT, B.OUT_AA, B.OUT_HEADS)


def test_the_library_is_built_next_to_the_others(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    assert os.path.basename(B.OUT_MASK) == "librip_mask_hip.so" and os.path.exists(B.OUT_MASK)
    assert os.path.dirname(B.OUT_MASK) == os.path.dirname(LIB_PATH)
    for name in ("rip_set_rect_mask", "rip_get_rect_mask_mode", "rip_get_output_mask", "rip_get_output_mask_device", "rip_debug_rect_mask_info"):
        assert hasattr(rip_lib, name), name


def test_the_table_is_exactly_the_librarys_kernels(rip_lib):
    from raw_image_pipeline_amd import build as B
    names = instantiations(B.OUT_MASK)
    assert all(count == 1 for count in names.values()), names
    records = {(name, 0) for name in names}
    table = set(MV.TABLE)
    assert not sorted(records - table), "kernels without a case (tests/mask_variant_cases.py): %s" % sorted(records - table)
    assert not sorted(table - records), "entries name kernels the library does not hold: %s" % sorted(table - records)
    assert set(names) == {"rect_mask_kernel<false>", "rect_mask_kernel<true>", "mask_threshold_kernel"}


def test_no_library_holds_a_kernel_of_another(rip_lib):
    from raw_image_pipeline_amd import build as B
    mine = set(instantiations(B.OUT_MASK))
    for so in others():
        theirs = set(instantiations(so))
        assert not [n for n in theirs if "rect_mask" in n or "mask_threshold" in n], so
        assert not (mine & theirs), so


def test_the_build_covers_the_mask_library(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    assert list(B.MASK_LIBRARIES) == ["mask"] and "mask" not in B.COMPANIONS and "mask" not in B.HEAD_LIBRARIES
    assert B._all_keys() == list(B.COMPANIONS) + list(B.HEAD_LIBRARIES) + ["mask"]
    assert B.up_to_date() and B.mask_up_to_date() and B.companions_up_to_date()
    for f in B.MASK_SOURCES + B.MASK_HEADERS:
        assert os.path.exists(os.path.join(B.CSRC, f))
    assert B.MASK_SOURCES == ["rip_mask.hip"] and "rip_mask.hpp" in B.MASK_HEADERS and "rip_round_map.hpp" in B.MASK_HEADERS
    assert "rip_mask.hpp" in B.HEADERS              # rip_handle.hpp includes it
    assert "rip_round_map.hpp" in B.HEADERS         # rip_remap_dev.hpp includes it: the remap kernels share the quantiser
    # up_to_date() looks at the library's file: older than its source, it is out of date
    src = os.path.join(B.CSRC, "rip_mask.hip")
    before = os.stat(B.OUT_MASK)
    try:
        os.utime(B.OUT_MASK, (before.st_atime, os.path.getmtime(src) - 10))
        assert not B.mask_up_to_date() and not B.companions_up_to_date() and not B.up_to_date()
    finally:
        os.utime(B.OUT_MASK, (before.st_atime, before.st_mtime))
    assert B.up_to_date()
    needed = subprocess.run(["readelf", "-d", LIB_PATH], capture_output=True, text=True).stdout
    assert "librip_mask_hip.so" in needed and "$ORIGIN" in needed


def test_one_definition_of_the_map_quantiser():
    """round_map lives in rip_round_map.hpp alone; the remap kernels' header and the mask kernel include it."""
    from raw_image_pipeline_amd import build as B
    defined = [f for f in sorted(os.listdir(B.CSRC)) if "int round_map(float" in open(os.path.join(B.CSRC, f)).read()]
    assert defined == ["rip_round_map.hpp"]
    for f in ("rip_remap_dev.hpp", "rip_mask.hip"):
        assert '#include "rip_round_map.hpp"' in open(os.path.join(B.CSRC, f)).read(), f
