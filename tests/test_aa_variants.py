"""The table of tests/aa_variant_cases.py is closed over the companion library librip_aa_hip.so: every instantiation of the
antialiased resize kernel has a case and every case names a kernel that exists; no other library holds an aa_kernel and the companion
holds none of theirs.  Reads the symbol tables (the host-side launch stubs) with the parser of tests/test_variant_cases.py; no
instruction stream."""
import os
import re

import aa_cases as AC
import aa_variant_cases as AV
from test_variant_cases import instantiations


def aa_path():
    from raw_image_pipeline_amd import build as B
    return B.OUT_AA


def test_the_companion_is_built_next_to_the_library(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    assert os.path.exists(aa_path())
    assert os.path.dirname(aa_path()) == os.path.dirname(LIB_PATH)
    assert hasattr(rip_lib, "rip_set_output_interpolation") and hasattr(rip_lib, "rip_debug_resize_aa_tables")


def test_the_table_is_exactly_the_companions_four_instantiations(rip_lib):
    names = instantiations(aa_path())
    assert all(count == 1 for count in names.values()), names
    records = {(name, 0) for name in names}
    table = set(AV.TABLE)
    missing = sorted(records - table)
    assert not missing, "instantiations without a case (tests/aa_variant_cases.py): %s" % missing
    stale = sorted(table - records)
    assert not stale, "entries name kernels the companion does not hold: %s" % stale
    assert len(AV.CASES) == 4
    assert {c.name for c in AV.CASES} == {AV.kernel_name(ch, w) for ch in (1, 3) for w in (False, True)}
    for c in AV.CASES:
        assert AC.kernel_name(c.channels, c.roi is not None) == c.name and c.filter in AC.FILTER_NAMES
    assert {c.filter for c in AV.CASES if c.roi} == set(AC.FILTER_NAMES) == {c.filter for c in AV.CASES if not c.roi}


def test_no_other_library_holds_an_aa_kernel(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    for so in (LIB_PATH, B.OUT_COMPANION, B.OUT_RSZ, B.OUT_AREA, B.OUT_FIT):
        assert not [n for n in instantiations(so) if "aa_kernel" in n], so
    assert not [n for n in instantiations(aa_path()) if "aa_kernel" not in n]


def test_up_to_date_covers_the_companion(rip_lib):
    from raw_image_pipeline_amd import build as B
    assert B.up_to_date() and B.aa_up_to_date()
    assert len(B.COMPANIONS) == 5 and B.COMPANIONS["aa"][0] == B.OUT_AA
    for f in B.AA_SOURCES + B.AA_HEADERS:
        assert os.path.exists(os.path.join(B.CSRC, f))
    assert "rip_aa.hpp" in B.HEADERS       # rip_handle.hpp includes it: librip_hip.so is rebuilt when the interface changes


def test_the_shapes_of_the_tests_come_from_the_headers_constants():
    import aa_reference as A
    from raw_image_pipeline_amd import build as B
    text = open(os.path.join(B.CSRC, "rip_aa.hpp")).read()
    const = lambda name: int(re.search(r"constexpr (?:int|size_t) %s = (\d+);" % name, text).group(1))
    assert (const("kAaTileCols"), const("kAaBlock"), const("kAaMaxTileRows")) == (AC.TILE_W, 256, 8) and A.TILE_W == AC.TILE_W
    assert const("kAaMaxFactor") == AC.MAX_FACTOR == A.MAX_FACTOR and const("kAaMaxSide") == 16384 and const("kAaMaxLdsBytes") == A.LDS_BYTES
