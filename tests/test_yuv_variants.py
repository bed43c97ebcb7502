"""The table of tests/yuv_variant_cases.py is closed over the library librip_yuv_hip.so: every kernel has a case and every case names a
kernel that exists, once each; no other library holds a yuv420 kernel and this one holds none of theirs.  Reads the symbol tables (the
host-side launch stubs) with the parser of tests/test_variant_cases.py; no instruction stream.  And the build: the fourth table of
raw_image_pipeline_amd/build.py, its dating and the link, with the three closed tables as they were."""
import os
import subprocess

import yuv_variant_cases as YV
from test_variant_cases import instantiations


def others():
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    return (LIB_PATH, B.OUT_COMPANION, B.OUT_RSZ, B.OUT_AREA, B.OUT_FIT, B.OUT_AA, B.OUT_HEADS, B.OUT_MASK)


def test_the_library_is_built_next_to_the_others(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    assert os.path.basename(B.OUT_YUV) == "librip_yuv_hip.so" and os.path.exists(B.OUT_YUV)
    assert os.path.dirname(B.OUT_YUV) == os.path.dirname(LIB_PATH)
    for name in ("rip_set_output_yuv_matrix", "rip_get_output_yuv_matrix"):
        assert hasattr(rip_lib, name), name


def test_the_table_is_exactly_the_librarys_kernels(rip_lib):
    from raw_image_pipeline_amd import build as B
    names = instantiations(B.OUT_YUV)
    assert all(count == 1 for count in names.values()), names
    records = {(name, 0) for name in names}
    table = set(YV.TABLE)
    assert not sorted(records - table), "kernels without a case (tests/yuv_variant_cases.py): %s" % sorted(records - table)
    assert not sorted(table - records), "entries name kernels the library does not hold: %s" % sorted(table - records)
    assert set(names) == {"yuv420_kernel<true>", "yuv420_kernel<false>"}


def test_no_library_holds_a_kernel_of_another(rip_lib):
    from raw_image_pipeline_amd import build as B
    mine = set(instantiations(B.OUT_YUV))
    for so in others():
        theirs = set(instantiations(so))
        assert not [n for n in theirs if "yuv420" in n], so
        assert not (mine & theirs), so


def test_the_build_covers_the_yuv_library(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    assert list(B.YUV_LIBRARIES) == ["yuv"] and not any("yuv" in t for t in B._tables())
    # the three closed tables are what they were; the link list is those and this one
    assert B._all_keys() == list(B.COMPANIONS) + list(B.HEAD_LIBRARIES) + ["mask"] and len(B.COMPANIONS) == 5
    assert B._link_keys() == B._all_keys() + ["yuv"]
    assert B.up_to_date() and B.yuv_up_to_date() and B.companions_up_to_date()
    for f in B.YUV_SOURCES + B.YUV_HEADERS:
        assert os.path.exists(os.path.join(B.CSRC, f))
    assert B.YUV_SOURCES == ["rip_yuv.hip"] and B.YUV_HEADERS == ["rip_yuv.hpp"]
    assert "rip_yuv.hpp" in B.HEADERS              # rip_handle.hpp includes it
    # up_to_date() looks at the library's file: older than its source, it is out of date
    src = os.path.join(B.CSRC, "rip_yuv.hip")
    before = os.stat(B.OUT_YUV)
    try:
        os.utime(B.OUT_YUV, (before.st_atime, os.path.getmtime(src) - 10))
        assert not B.yuv_up_to_date() and not B.companions_up_to_date() and not B.up_to_date()
    finally:
        os.utime(B.OUT_YUV, (before.st_atime, before.st_mtime))
    assert B.up_to_date()
    needed = subprocess.run(["readelf", "-d", LIB_PATH], capture_output=True, text=True).stdout
    assert "librip_yuv_hip.so" in needed and "$ORIGIN" in needed
