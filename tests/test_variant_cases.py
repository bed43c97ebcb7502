"""The table of tests/variant_cases.py is closed over the library: every kernel instantiation of the built librip_hip.so has a
case, is listed as unreachable with its proof, or is measurement code -- and nothing in the table names a kernel that does not
exist.  Reads the symbol table (the host-side launch stubs, one per instantiation and translation unit); no instruction stream."""
import collections
import os
import re
import shutil
import subprocess

import pytest

import variant_cases as V


def readelf():
    from raw_image_pipeline_amd import build as B
    hipcc = shutil.which(B.hipcc()) or B.hipcc()
    root = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for cand in (os.path.join(root, "llvm", "bin", "llvm-readelf"), os.path.join(root, "lib", "llvm", "bin", "llvm-readelf"),
                 "/opt/rocm/llvm/bin/llvm-readelf", shutil.which("llvm-readelf")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("llvm-readelf not found next to hipcc")


def instantiations(so):
    """Counter of the kernels' names, template arguments included, namespaces stripped -- as the launch log spells them."""
    text = subprocess.run([readelf(), "-sW", "--demangle", so], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    names = collections.Counter()
    for line in text.splitlines():
        if "__device_stub__" not in line:
            continue
        sym = line.split("__device_stub__", 1)[1]
        sym = sym.replace("rip::", "").replace("(anonymous namespace)::", "")
        depth, end = 0, None
        for i, ch in enumerate(sym):   # the name ends at the parenthesis of the parameter list, outside the template arguments
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                end = i
                break
        assert end is not None, line
        names[sym[:end]] += 1
    return names


@pytest.fixture(scope="module")
def library_records(rip_lib):
    from raw_image_pipeline_amd import LIB_PATH
    records = set()
    for name, count in instantiations(LIB_PATH).items():
        assert count in (1, 2), "%s is compiled %d times" % (name, count)
        records.add((name, 0))
        if count == 2:   # compiled again under the contracted model: the twin shares the name
            records.add((name, 1))
    return records


def test_the_table_is_exactly_the_librarys_instantiations(library_records):
    table, unreachable, probes = set(V.TABLE), set(V.UNREACHABLE), set(V.NOT_PRODUCT)
    assert not (table & unreachable) and not (table & probes) and not (unreachable & probes), "the three sets overlap"
    missing = sorted(library_records - table - unreachable - probes)
    assert not missing, "%d instantiations without a case (tests/variant_cases.py): %s" % (len(missing), missing[:12])
    stale = sorted((table | unreachable | probes) - library_records)
    assert not stale, "%d entries name kernels the library does not hold: %s" % (len(stale), stale[:12])


def test_unreachable_entries_carry_their_proof():
    for record, proof in V.UNREACHABLE.items():
        assert re.search(r"rip_\w+\.(hip|cpp|hpp)", proof) and len(proof) > 40, "%s: name the dispatch line that rules it out" % (record,)


def test_cases_are_well_formed():
    import packed_reference as R
    assert len(V.CASES) == len(V.TABLE)
    for c in V.CASES:
        assert c.fc in (0, 1) and c.sizes and c.n_frames >= 3, c
        assert c.source in ("bayer8", "bgr8", "mono8", "bayer16", "raw16", "packed"), c
        assert (c.range16 is not None) == (c.source in ("raw16", "packed")), c
        if c.source == "packed":
            assert all(R.allowed_width(w, c.layout) == w for w, _ in c.sizes), c
        if c.cfg.get("undistort"):
            assert c.camera is not None, c
        # no neutral stage parameters (a stage that does nothing hides a wrong branch)
        if c.cfg.get("cc"):
            assert any(c.cfg["cc_bias"]), c
        if c.cfg.get("gamma"):
            assert c.cfg["gamma_k"] != 1.0, c
        if c.cfg.get("ce"):
            assert (c.cfg["ce_hue"], c.cfg["ce_sat"], c.cfg["ce_val"]) == (1.3, 0.7, 1.1), c
    assert sum(c.single_frame for c in V.CASES) == 3


def test_stub_names_are_parsed():
    line = "  1: 0 85 FUNC LOCAL DEFAULT 13 void rip::(anonymous namespace)::__device_stub__raw16_tile_kernel<rip::(anonymous namespace)::StagePacked<1>, true, 0, 0, 90>(rip::Raw16Params)"
    sym = line.split("__device_stub__", 1)[1].replace("rip::", "").replace("(anonymous namespace)::", "")
    assert sym.startswith("raw16_tile_kernel<StagePacked<1>, true, 0, 0, 90>(")
    assert ("raw16_tile_kernel<StagePacked<1>, true, 0, 0, 90>", 0) in V.TABLE
