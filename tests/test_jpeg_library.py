"""librip_jpeg_hip.so, the row of raw_image_pipeline_amd/build.py's third table ENCODER_LIBRARIES: the table is closed, the library
holds exactly the kernels of tests/jpeg_variant_cases.py, no other library holds a jpeg_ kernel, up_to_date() dates it and
librip_hip.so links it through $ORIGIN behind the other two tables.  Reads the symbol tables with the parser of
tests/test_variant_cases.py; no instruction stream."""
import os
import subprocess

import jpeg_variant_cases as JV
from test_variant_cases import instantiations


def test_the_third_table_holds_exactly_this_library_and_leaves_the_others_alone():
    from raw_image_pipeline_amd import build as B
    assert [c.key for c in B.ENCODER_LIBRARIES] == ["jpeg"]
    row = B.ENCODER_LIBRARIES[0]
    assert type(row) is B.Companion and B.kernel_library("jpeg") == row
    assert os.path.basename(row.out) == "librip_jpeg_hip.so" and os.path.dirname(row.out) == os.path.dirname(B.OUT)
    assert row.sources == ["rip_jpeg.hip"] and set(row.headers) == {"rip_jpeg.hpp", "rip_jpeg_dev.hpp", "rip_yuv.hpp"} and row.build_dir == "build_jpeg"
    for f in row.sources + row.headers:
        assert os.path.exists(os.path.join(B.CSRC, f)), f
    assert "rip_jpeg.hpp" in B.HEADERS and "rip_jpeg_dev.hpp" not in B.HEADERS      # librip_hip.so sees the interface alone
    assert "jpeg" not in [c.key for c in B.COMPANIONS + B.STAGE_LIBRARIES] and len(B.COMPANIONS) == 8 and [c.key for c in B.STAGE_LIBRARIES] == ["clahe"]
    assert [B.kernel_library(c.key) for c in B.COMPANIONS + B.STAGE_LIBRARIES] == list(B.COMPANIONS + B.STAGE_LIBRARIES)


def test_the_library_holds_exactly_the_tables_instantiations(rip_lib):
    from raw_image_pipeline_amd import build as B
    names = instantiations(B.kernel_library("jpeg").out)
    assert names and all(count == 1 for count in names.values()), names
    assert {(name, 0) for name in names} == set(JV.TABLE)
    for entry in ("rip_set_output_jpeg", "rip_get_output_jpeg", "rip_get_output_jpeg_sizes", "rip_get_output_jpeg_sizes_device", "rip_debug_jpeg_tables"):
        assert hasattr(rip_lib, entry), entry


def test_no_other_library_holds_a_jpeg_kernel(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    for so in [c.out for c in B.COMPANIONS + B.STAGE_LIBRARIES] + [LIB_PATH]:
        assert not [n for n in instantiations(so) if "jpeg" in n], so


def test_the_core_library_links_it_through_origin_behind_the_other_tables(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    needed = subprocess.run(["readelf", "-d", LIB_PATH], capture_output=True, text=True).stdout
    assert "librip_jpeg_hip.so" in needed and "$ORIGIN" in needed
    order = [needed.index(os.path.basename(c.out)) for c in B.COMPANIONS + B.STAGE_LIBRARIES + B.ENCODER_LIBRARIES]
    assert order == sorted(order)
    soname = subprocess.run(["readelf", "-d", B.kernel_library("jpeg").out], capture_output=True, text=True).stdout
    assert "librip_jpeg_hip.so" in soname


def test_up_to_date_looks_at_the_librarys_file(rip_lib):
    """Older than its source, the library is out of date -- for its own check, for the check of its table and for up_to_date(); the
    checks of the other two tables keep their meaning."""
    from raw_image_pipeline_amd import build as B
    row = B.kernel_library("jpeg")
    fresh = lambda: (B.up_to_date(), B.companion_up_to_date("jpeg"), B.encoder_libraries_up_to_date(), B.stage_libraries_up_to_date(), B.companions_up_to_date())
    assert fresh() == (True, True, True, True, True)
    before = os.stat(row.out)
    try:
        os.utime(row.out, (before.st_atime, min(os.path.getmtime(os.path.join(B.CSRC, f)) for f in row.sources + row.headers) - 10))
        assert fresh() == (False, False, False, True, True)
    finally:
        os.utime(row.out, (before.st_atime, before.st_mtime))
    assert fresh() == (True, True, True, True, True)
