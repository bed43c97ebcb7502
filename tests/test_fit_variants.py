"""The table of tests/fit_variant_cases.py is closed over the companion library librip_fit_hip.so: every instantiation of its kernels
has a case and every case names a kernel that exists; the companion holds no kernel of the other libraries' names and they hold none
of its.  Reads the symbol tables (the host-side launch stubs) with the parser of tests/test_variant_cases.py; no instruction stream."""
import os

import fit_cases as FC
import fit_variant_cases as FV
from test_variant_cases import instantiations


def fit_path():
    from raw_image_pipeline_amd import build as B
    return B.OUT_FIT


def test_the_companion_is_built_next_to_the_library(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    assert os.path.exists(fit_path())
    assert os.path.dirname(fit_path()) == os.path.dirname(LIB_PATH)
    for name in ("rip_set_output_roi", "rip_set_output_fit", "rip_set_output_pad", "rip_get_output_window", "rip_debug_output_window"):
        assert hasattr(rip_lib, name), name


def test_the_table_is_exactly_the_companions_instantiations(rip_lib):
    names = instantiations(fit_path())
    assert all(count == 1 for count in names.values()), names
    records = {(name, 0) for name in names}
    table = set(FV.TABLE)
    missing = sorted(records - table)
    assert not missing, "instantiations without a case (tests/fit_variant_cases.py): %s" % missing
    stale = sorted(table - records)
    assert not stale, "entries name kernels the companion does not hold: %s" % stale
    assert len(FV.CASES) == 10
    for v in FV.CASES:
        name, padded = FC.kernel_of(v.case)
        assert v.name == ("fit_pad_kernel<%d>" % v.case.channels if padded else name), v


def test_the_libraries_keep_their_kernels_apart(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    from raw_image_pipeline_amd import build as B
    for so in (LIB_PATH, B.OUT_COMPANION, B.OUT_RSZ, B.OUT_AREA):
        assert not [n for n in instantiations(so) if n.startswith("fit_")], so
    assert not [n for n in instantiations(fit_path()) if "resize_kernel" in n or "area_reduce_kernel" in n or "output_convert" in n]


def test_up_to_date_covers_the_companion(rip_lib):
    from raw_image_pipeline_amd import build as B
    assert B.up_to_date() and B.fit_up_to_date()
    for f in B.FIT_SOURCES + B.FIT_HEADERS:
        assert os.path.exists(os.path.join(B.CSRC, f))
    assert "rip_fit.hpp" in B.HEADERS      # rip_handle.hpp includes it: librip_hip.so is rebuilt when the interface changes
