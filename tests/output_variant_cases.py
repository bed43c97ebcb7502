"""One case per kernel instantiation of the companion library librip_out_hip.so (csrc/rip_output.hip): which output format makes
exactly that converter run.  tests/test_output_variants.py (CPU) checks that the table is exactly the companion's
instantiations -- in both directions -- and that librip_hip.so has gained none; tests/test_output_format_gpu.py runs every case,
reads the handle's launch log and compares the delivered tensor with tests/output_reference.py.

Importable without a GPU; nothing here looks at the library.  ``mono8`` on a one-channel result is the identity and has no kernel.

Size (w, h) = (1027, 5): two workgroups of 1024 pixels per row, the second one ragged with a last lane of 3 pixels; an odd width
makes tight planes change their alignment from row to row."""
import collections

SIZE = (1027, 5)

Case = collections.namedtuple("Case", ["name", "fc", "format", "size", "n_frames", "norm"])

# (format name of rip_set_output_format, the tag type of rip_output.hip)
FORMAT_TAGS = (("rgb8", "Rgb8"), ("mono8", "Mono8"), ("rgb_chw_f32", "RgbChwF32"), ("rgb_chw_f16", "RgbChwF16"),
               ("rgb_chw_bf16", "RgbChwBf16"), ("bgr_chw_f32", "BgrChwF32"), ("bgr_chw_f16", "BgrChwF16"),
               ("bgr_chw_bf16", "BgrChwBf16"))
# a normalisation with three different planes, so that a swapped plane or table row shows
NORM = (255.0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))

CASES = [Case("output_convert_kernel<%s>" % tag, 0, fmt, SIZE, 3, NORM) for fmt, tag in FORMAT_TAGS]
TABLE = {(c.name, c.fc): c for c in CASES}
assert len(TABLE) == len(CASES), "two cases for one record"
KERNEL_OF_FORMAT = {c.format: c.name for c in CASES}


def case_id(case):
    return case.name
