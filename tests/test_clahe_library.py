"""librip_clahe_hip.so, the row of raw_image_pipeline_amd/build.py's second table STAGE_LIBRARIES: the table is closed, the library
holds exactly the kernels of tests/clahe_variant_cases.py, no other library holds a clahe_ kernel, up_to_date() dates it and
librip_hip.so links it through $ORIGIN.  Reads the symbol tables with the parser of tests/test_variant_cases.py; no instruction
stream."""
import os
import subprocess

import clahe_variant_cases as CV
from test_variant_cases import instantiations


def test_the_second_table_holds_exactly_this_library_and_leaves_the_first_alone():
    from raw_image_pipeline_amd import build as B
    assert [c.key for c in B.STAGE_LIBRARIES] == ["clahe"]
    row = B.STAGE_LIBRARIES[0]
    assert type(row) is B.Companion and B.kernel_library("clahe") == row
    assert os.path.basename(row.out) == "librip_clahe_hip.so" and os.path.dirname(row.out) == os.path.dirname(B.OUT)
    assert row.sources == ["rip_clahe.hip"] and set(row.headers) == {"rip_clahe.hpp", "rip_clahe_dev.hpp"} and row.build_dir == "build_clahe"
    for f in row.sources + row.headers:
        assert os.path.exists(os.path.join(B.CSRC, f)), f
    assert "rip_clahe.hpp" in B.HEADERS and "rip_clahe_dev.hpp" not in B.HEADERS      # librip_hip.so sees the interface alone
    assert "clahe" not in [c.key for c in B.COMPANIONS] and len(B.COMPANIONS) == 8
    assert [B.kernel_library(c.key) for c in B.COMPANIONS] == list(B.COMPANIONS)


def test_the_library_holds_exactly_the_tables_instantiations(rip_lib):
    from raw_image_pipeline_amd import build as B
    names = instantiations(B.kernel_library("clahe").out)
    assert names and all(count == 1 for count in names.values()), names
    assert {(name, 0) for name in names} == set(CV.TABLE)
    assert hasattr(rip_lib, "rip_set_output_clahe") and hasattr(rip_lib, "rip_get_output_clahe")


def test_no_other_library_holds_a_clahe_kernel(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    for so in [c.out for c in B.COMPANIONS] + [LIB_PATH]:
        assert not [n for n in instantiations(so) if "clahe" in n], so


def test_the_core_library_links_it_through_origin_behind_the_companions(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    needed = subprocess.run(["readelf", "-d", LIB_PATH], capture_output=True, text=True).stdout
    assert "librip_clahe_hip.so" in needed and "$ORIGIN" in needed
    order = [needed.index(os.path.basename(c.out)) for c in B.COMPANIONS + B.STAGE_LIBRARIES]
    assert order == sorted(order)
    soname = subprocess.run(["readelf", "-d", B.kernel_library("clahe").out], capture_output=True, text=True).stdout
    assert "librip_clahe_hip.so" in soname


def test_up_to_date_looks_at_the_librarys_file(rip_lib):
    """Older than its source, the library is out of date -- for its own check, for the check of its table and for up_to_date(); the
    companions' check keeps its meaning."""
    from raw_image_pipeline_amd import build as B
    row = B.kernel_library("clahe")
    fresh = lambda: (B.up_to_date(), B.companion_up_to_date("clahe"), B.stage_libraries_up_to_date(), B.companions_up_to_date())
    assert fresh() == (True, True, True, True)
    before = os.stat(row.out)
    try:
        os.utime(row.out, (before.st_atime, os.path.getmtime(os.path.join(B.CSRC, row.sources[0])) - 10))
        assert fresh() == (False, False, False, True)
    finally:
        os.utime(row.out, (before.st_atime, before.st_mtime))
    assert fresh() == (True, True, True, True)
