"""One case per kernel instantiation of the companion library librip_fit_hip.so (csrc/rip_fit.hip): a final image, a window of it, a
target, a fit mode and an interpolation that make exactly that kernel run (tests/fit_cases.py Case).  tests/test_fit_variants.py
(CPU) checks that the table is exactly the companion's instantiations -- in both directions; tests/test_fit_gpu.py runs every case,
reads the handle's launch log and compares the delivered frames with tests/fit_reference.py.

Importable without a GPU; nothing here looks at the library.

The resize cases read a 130 x 19 window at (3, 2) of a 140 x 23 image -- byte phase 1 with three channels, 3 with one -- and write
more than one workgroup of the area kernels per axis; the pad cases letterbox all of a 40 x 10 image into 33 x 33."""
import collections

import fit_cases as FC

Variant = collections.namedtuple("Variant", ["name", "fc", "case"])

SIZE, ROI = (140, 23), (3, 2, 130, 19)
TARGETS = {"fit_linear_kernel<%d>": ("linear", (77, 11)), "fit_mean2_kernel<%d>": ("linear", (65, 0)),
           "fit_area_kernel<%d, true>": ("area", (26, 19)), "fit_area_kernel<%d, false>": ("area", (87, 13))}


def _cases():
    out = []
    for cn in (1, 3):
        for name, (interp, target) in sorted(TARGETS.items()):
            roi = ROI if target[1] else (3, 2, 130, 18)           # the mean halves both sides
            target = target if target[1] else (65, 9)
            out.append(Variant(name % cn, 0, FC.case(cn, SIZE, roi, target, "stretch", interp, n=3)))
        out.append(Variant("fit_pad_kernel<%d>" % cn, 0, FC.case(cn, (40, 10), None, (33, 33), "letterbox", "linear", FC.PADS[2], n=3)))
    return out


CASES = _cases()
TABLE = {(v.name, v.fc): v for v in CASES}
assert len(TABLE) == len(CASES), "two cases for one record"


def case_id(v):
    return v.name
