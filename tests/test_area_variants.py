"""The table of tests/area_variant_cases.py is closed over the companion library librip_area_hip.so: every instantiation of the area
kernel has a case and every case names a kernel that exists; the three other libraries hold none of its kernels.  Reads the symbol
tables (the host-side launch stubs) with the parser of tests/test_variant_cases.py; no instruction stream."""
import os
import re

import area_cases as AC
import area_variant_cases as AV
from test_variant_cases import instantiations


def area_path():
    from raw_image_pipeline_amd import build as B
    return B.OUT_AREA


def test_the_companion_is_built_next_to_the_library(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    assert os.path.exists(area_path())
    assert os.path.dirname(area_path()) == os.path.dirname(LIB_PATH)
    assert hasattr(rip_lib, "rip_set_output_interpolation") and hasattr(rip_lib, "rip_debug_resize_area_tables")


def test_the_table_is_exactly_the_companions_instantiations(rip_lib):
    names = instantiations(area_path())
    assert all(count == 1 for count in names.values()), names
    records = {(name, 0) for name in names}
    table = set(AV.TABLE)
    missing = sorted(records - table)
    assert not missing, "instantiations without a case (tests/area_variant_cases.py): %s" % missing
    stale = sorted(table - records)
    assert not stale, "entries name kernels the companion does not hold: %s" % stale
    assert len(AV.CASES) == 4
    assert {c.name for c in AV.CASES} == {AV.kernel_name(ch, w) for ch in (1, 3) for w in (False, True)}
    for c in AV.CASES:
        assert AC.kernel_name(c.channels, AC.kind_of(c.src_size, c.dst_size)) == c.name


def test_the_other_libraries_hold_no_area_kernel(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    for so in (LIB_PATH, B.OUT_COMPANION, B.OUT_RSZ):
        assert not [n for n in instantiations(so) if "area_reduce_kernel" in n], so
    assert not [n for n in instantiations(area_path()) if "resize_kernel" in n]


def test_up_to_date_covers_the_companion(rip_lib):
    from raw_image_pipeline_amd import build as B
    assert B.up_to_date() and B.area_up_to_date()
    for f in B.AREA_SOURCES + B.AREA_HEADERS:
        assert os.path.exists(os.path.join(B.CSRC, f))
    assert "rip_area.hpp" in B.HEADERS     # rip_handle.hpp includes it: librip_hip.so is rebuilt when the interface changes


def test_the_shapes_of_the_tests_come_from_the_headers_constants():
    from raw_image_pipeline_amd import build as B
    text = open(os.path.join(B.CSRC, "rip_area.hpp")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert (const("kAreaTileCols"), const("kAreaTileRows"), const("kAreaBlock")) == (AC.TILE_W, AC.TILE_H, 256)
    assert const("kAreaMaxFactor") == 256 and const("kAreaMaxSide") == 16384
