"""The kernel libraries of raw_image_pipeline_amd/build.py's one table KERNEL_LIBRARIES: the table itself is closed, every library's
tests/*_variant_cases.py table is closed over that library's kernels, no library holds a kernel of another, every library is dated by
up_to_date() and linked by librip_hip.so in the table's order.  Reads the symbol tables (the host-side launch stubs) with the parser of
tests/test_variant_cases.py; no instruction stream."""
import collections
import importlib
import itertools
import os
import re
import subprocess

import pytest

import variant_cases as V
from test_variant_cases import instantiations

# Per key: the case module, the C-ABI names the library stands behind, the interface header rip_handle.hpp includes (librip_hip.so is
# rebuilt when it changes), the stems of the library's kernel names ("^..." is a prefix, anything else a substring) and the row of
# build.py as literals.
Lib = collections.namedtuple("Lib", "cases abi header stems so sources headers")
RESIZE_SHARED = ["rip_resize_dev.hpp", "rip_resize.hpp", "rip_area.hpp", "rip_launch_info.hpp"]
LIBS = collections.OrderedDict([
    ("out", Lib("output_variant_cases", ["rip_set_output_format"], "rip_output.hpp", ["output_convert"],
                "librip_out_hip.so", ["rip_output.hip"], ["rip_output.hpp", "rip_launch_info.hpp"])),
    ("rsz", Lib("resize_variant_cases", ["rip_set_output_size"], "rip_resize.hpp", ["resize_kernel"],
                "librip_rsz_hip.so", ["rip_resize.hip"], RESIZE_SHARED)),
    ("area", Lib("area_variant_cases", ["rip_set_output_interpolation", "rip_debug_resize_area_tables"], "rip_area.hpp", ["area_reduce_kernel"],
                 "librip_area_hip.so", ["rip_area.hip"], RESIZE_SHARED)),
    ("fit", Lib("fit_variant_cases", ["rip_set_output_roi", "rip_set_output_fit", "rip_set_output_pad", "rip_get_output_window", "rip_debug_output_window"],
                "rip_fit.hpp", ["^fit_"], "librip_fit_hip.so", ["rip_fit.hip"], ["rip_fit.hpp"] + RESIZE_SHARED)),
    ("aa", Lib("aa_variant_cases", ["rip_set_output_interpolation", "rip_debug_resize_aa_tables"], "rip_aa.hpp", ["aa_kernel"],
               "librip_aa_hip.so", ["rip_aa.hip"], ["rip_aa.hpp", "rip_aa_dev.hpp"] + RESIZE_SHARED)),
    ("heads", Lib("heads_variant_cases", ["rip_apply_device_heads", "rip_debug_output_head_info"], "rip_heads.hpp", ["head_copy_kernel"],
                  "librip_heads_hip.so", ["rip_heads.hip"], ["rip_heads.hpp", "rip_launch_info.hpp"])),
    ("mask", Lib("mask_variant_cases", ["rip_set_rect_mask", "rip_get_rect_mask_mode", "rip_get_output_mask", "rip_get_output_mask_device", "rip_debug_rect_mask_info"],
                 "rip_mask.hpp", ["rect_mask", "mask_threshold"], "librip_mask_hip.so", ["rip_mask.hip"], ["rip_mask.hpp", "rip_round_map.hpp", "rip_launch_info.hpp"])),
    ("yuv", Lib("yuv_variant_cases", ["rip_set_output_yuv_matrix", "rip_get_output_yuv_matrix"], "rip_yuv.hpp", ["yuv420"],
                "librip_yuv_hip.so", ["rip_yuv.hip"], ["rip_yuv.hpp", "rip_launch_info.hpp"])),
    ("clahe", Lib("clahe_variant_cases", ["rip_set_output_clahe", "rip_get_output_clahe"], "rip_clahe.hpp", ["clahe_"],
                  "librip_clahe_hip.so", ["rip_clahe.hip"], ["rip_clahe.hpp", "rip_clahe_dev.hpp", "rip_launch_info.hpp"])),
    ("jpeg", Lib("jpeg_variant_cases", ["rip_set_output_jpeg", "rip_get_output_jpeg", "rip_get_output_jpeg_sizes", "rip_get_output_jpeg_sizes_device", "rip_debug_jpeg_tables"],
                 "rip_jpeg.hpp", ["jpeg_"], "librip_jpeg_hip.so", ["rip_jpeg.hip"], ["rip_jpeg.hpp", "rip_jpeg_dev.hpp", "rip_yuv.hpp", "rip_launch_info.hpp"])),
])
KEYS = list(LIBS)
CORE = "librip_hip.so"


def matches(name, stems):
    return any(name.startswith(s[1:]) if s.startswith("^") else s in name for s in stems)


@pytest.fixture(scope="module")
def kernels(rip_lib):
    """Counter of the kernel instantiations of each of the eleven libraries, read once."""
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    found = {c.key: instantiations(c.out) for c in B.KERNEL_LIBRARIES}
    found[CORE] = instantiations(LIB_PATH)
    return found


# ---- the table -----------------------------------------------------------------------------------------------------------------
def test_the_table_holds_exactly_these_libraries_in_link_order():
    from raw_image_pipeline_amd import build as B
    assert [c.key for c in B.KERNEL_LIBRARIES] == KEYS == ["out", "rsz", "area", "fit", "aa", "heads", "mask", "yuv", "clahe", "jpeg"]
    assert [B.kernel_library(k) for k in KEYS] == list(B.KERNEL_LIBRARIES) and all(type(c) is B.KernelLibrary for c in B.KERNEL_LIBRARIES)
    assert "rip_round_map.hpp" in B.HEADERS         # rip_remap_dev.hpp includes it: the remap kernels share the quantiser
    assert "rip_round_map.hpp" in B.kernel_library("mask").headers


@pytest.mark.parametrize("key", KEYS)
def test_the_row_is_what_it_was_and_its_files_exist(rip_lib, key):
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    row, lib = B.kernel_library(key), LIBS[key]
    assert os.path.basename(row.out) == lib.so and row.sources == lib.sources and set(row.headers) == set(lib.headers)
    assert row.build_dir == "build_" + key
    assert os.path.exists(row.out) and os.path.dirname(row.out) == os.path.dirname(LIB_PATH)
    for f in row.sources + row.headers:
        assert os.path.exists(os.path.join(B.CSRC, f)), f
    assert lib.header in row.headers and lib.header in B.HEADERS
    assert not [h for h in row.headers if h.endswith("_dev.hpp") and h in B.HEADERS]      # librip_hip.so sees the interface alone
    assert "rip_launch_info.hpp" in row.headers and "rip_launch_info.hpp" in B.HEADERS
    for name in lib.abi:
        assert hasattr(rip_lib, name), name


# ---- case table = kernels, both ways ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_the_case_table_is_exactly_the_librarys_instantiations(kernels, key):
    names = kernels[key]
    assert names and all(count == 1 for count in names.values()), names
    records = {(name, 0) for name in names}
    table = set(importlib.import_module(LIBS[key].cases).TABLE)
    missing = sorted(records - table)
    assert not missing, "instantiations without a case (tests/%s.py): %s" % (LIBS[key].cases, missing)
    stale = sorted(table - records)
    assert not stale, "entries name kernels the library does not hold: %s" % stale


# ---- kernels kept apart ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_the_librarys_kernels_carry_its_stems_and_no_other_librarys_do(kernels, key):
    stems = LIBS[key].stems
    strangers = [n for n in kernels[key] if not matches(n, stems)]
    assert not strangers, "kernels of %s outside its stems %s: %s" % (key, stems, strangers)
    for other, names in kernels.items():
        if other != key:
            assert not [n for n in names if matches(n, stems)], other


def test_no_two_libraries_hold_the_same_instantiation(kernels):
    assert len(kernels) == 11
    for a, b in itertools.combinations(kernels, 2):
        assert not (set(kernels[a]) & set(kernels[b])), (a, b)


def test_the_core_library_has_gained_no_kernel(kernels):
    names = kernels[CORE]
    assert not [n for n in names if "output_convert" in n]
    records = set()
    for name, count in names.items():
        records.add((name, 0))
        if count == 2:
            records.add((name, 1))
    assert len(records) == len(V.TABLE) + len(V.NOT_PRODUCT) + len(V.UNREACHABLE)


# ---- dating and link ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_up_to_date_looks_at_the_librarys_file(rip_lib, key):
    """Older than its sources and headers, the library is out of date -- for its own check, for the check of all and for
    up_to_date(); every other library's own check keeps its meaning."""
    from raw_image_pipeline_amd import build as B
    row = B.kernel_library(key)
    others = [k for k in KEYS if k != key]
    fresh = lambda: (B.up_to_date(), B.kernel_library_up_to_date(key), B.kernel_libraries_up_to_date(), [B.kernel_library_up_to_date(k) for k in others])
    assert fresh() == (True, True, True, [True] * 9)
    before = os.stat(row.out)
    try:
        os.utime(row.out, (before.st_atime, min(os.path.getmtime(os.path.join(B.CSRC, f)) for f in row.sources + row.headers) - 10))
        assert fresh() == (False, False, False, [True] * 9)
    finally:
        os.utime(row.out, (before.st_atime, before.st_mtime))
    assert fresh() == (True, True, True, [True] * 9)


@pytest.mark.parametrize("key", KEYS)
def test_the_core_library_links_the_library_through_origin(rip_lib, key):
    """... in the table's order, and the library carries its own file name as its soname."""
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    needed = subprocess.run(["readelf", "-d", LIB_PATH], capture_output=True, text=True).stdout
    assert LIBS[key].so in needed and "$ORIGIN" in needed
    assert re.findall(r"\(NEEDED\).*\[(librip_\w+_hip\.so)\]", needed) == [lib.so for lib in LIBS.values()]
    own = subprocess.run(["readelf", "-d", B.kernel_library(key).out], capture_output=True, text=True).stdout
    assert re.findall(r"\(SONAME\).*\[(.*)\]", own) == [LIBS[key].so]


# ---- what each library's cases promise beyond their names --------------------------------------------------------------------------
def test_out_cases_cover_every_format():
    import output_variant_cases as OV
    assert len(OV.CASES) == 8 and {c.format for c in OV.CASES} == {f for f, _ in OV.FORMAT_TAGS}


def test_rsz_cases_are_the_cross_product():
    import resize_variant_cases as RV
    assert len(RV.CASES) == 4
    assert {c.name for c in RV.CASES} == {RV.kernel_name(ch, a) for ch in (1, 3) for a in (False, True)}


def test_area_cases_are_the_cross_product_and_named_by_their_sizes():
    import area_cases as AC
    import area_variant_cases as AV
    assert len(AV.CASES) == 4
    assert {c.name for c in AV.CASES} == {AV.kernel_name(ch, w) for ch in (1, 3) for w in (False, True)}
    for c in AV.CASES:
        assert AC.kernel_name(c.channels, AC.kind_of(c.src_size, c.dst_size)) == c.name


def test_area_shapes_come_from_the_headers_constants():
    import area_cases as AC
    from raw_image_pipeline_amd import build as B
    text = open(os.path.join(B.CSRC, "rip_area.hpp")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert (const("kAreaTileCols"), const("kAreaTileRows"), const("kAreaBlock")) == (AC.TILE_W, AC.TILE_H, 256)
    assert const("kAreaMaxFactor") == 256 and const("kAreaMaxSide") == 16384


def test_fit_cases_are_ten_and_padded_ones_name_the_pad_kernel():
    import fit_cases as FC
    import fit_variant_cases as FV
    assert len(FV.CASES) == 10
    for v in FV.CASES:
        name, padded = FC.kernel_of(v.case)
        assert v.name == ("fit_pad_kernel<%d>" % v.case.channels if padded else name), v


def test_aa_cases_are_the_cross_product_and_cover_both_filters():
    import aa_cases as AC
    import aa_variant_cases as AV
    assert len(AV.CASES) == 4
    assert {c.name for c in AV.CASES} == {AV.kernel_name(ch, w) for ch in (1, 3) for w in (False, True)}
    for c in AV.CASES:
        assert AC.kernel_name(c.channels, c.roi is not None) == c.name and c.filter in AC.FILTER_NAMES
    assert {c.filter for c in AV.CASES if c.roi} == set(AC.FILTER_NAMES) == {c.filter for c in AV.CASES if not c.roi}


def test_aa_shapes_come_from_the_headers_constants():
    import aa_cases as AC
    import aa_reference as A
    from raw_image_pipeline_amd import build as B
    text = open(os.path.join(B.CSRC, "rip_aa.hpp")).read()
    const = lambda name: int(re.search(r"constexpr (?:int|size_t) %s = (\d+);" % name, text).group(1))
    assert (const("kAaTileCols"), const("kAaBlock"), const("kAaMaxTileRows")) == (AC.TILE_W, 256, 8) and A.TILE_W == AC.TILE_W
    assert const("kAaMaxFactor") == AC.MAX_FACTOR == A.MAX_FACTOR and const("kAaMaxSide") == 16384 and const("kAaMaxLdsBytes") == A.LDS_BYTES


def test_heads_holds_one_kernel_and_its_cases_copy_identity_heads(kernels):
    import heads_cases as HC
    import heads_variant_cases as HV
    assert set(kernels["heads"]) == {"head_copy_kernel"}
    for c in HV.CASES:
        heads = HC.BY_NAME[c.head_set].heads
        assert all(heads[k] == HC.IDENTITY for k in c.copied_heads)


def test_mask_holds_exactly_three_kernels(kernels):
    assert set(kernels["mask"]) == {"rect_mask_kernel<false>", "rect_mask_kernel<true>", "mask_threshold_kernel"}


def test_one_definition_of_the_map_quantiser():
    """round_map lives in rip_round_map.hpp alone; the remap kernels' header and the mask kernel include it."""
    from raw_image_pipeline_amd import build as B
    defined = [f for f in sorted(os.listdir(B.CSRC)) if "int round_map(float" in open(os.path.join(B.CSRC, f)).read()]
    assert defined == ["rip_round_map.hpp"]
    for f in ("rip_remap_dev.hpp", "rip_mask.hip"):
        assert '#include "rip_round_map.hpp"' in open(os.path.join(B.CSRC, f)).read(), f


def test_yuv_holds_exactly_two_kernels(kernels):
    assert set(kernels["yuv"]) == {"yuv420_kernel<true>", "yuv420_kernel<false>"}
