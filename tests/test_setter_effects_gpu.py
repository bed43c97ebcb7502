"""What a setting change leaves behind on a live handle, in build counts: every output setter of the selected head, load_params and
set_output_heads is called with the value it already holds, with another valid value and with a refused one, and after a delivery
behind each the growth of the table builds (debug_output_head_info(k)[0]) and of the mask builds (debug_rect_mask_info(k)) of both
heads is compared with literal numbers.  The numbers were recorded from the library as it stood before the setters moved to
rip_settings.cpp and the invalidation helpers of rip_constants.cpp replaced the flag lists; they pin, among others, that an output
setter drops the head's delivered mask even when the call is then refused, that set_output_normalization always rebuilds the table
and that set_output_format rebuilds it only when the name changes."""
import pytest

from helpers import cfg, configure
from raw_image_pipeline_amd import RawImagePipeline, synth

pytestmark = pytest.mark.gpu
W, H, ENC = 64, 48, "bayer_rggb8"

PARAMS = """debayer:
  enabled: true
undistortion:
  enabled: true
  mask: coverage
output:
  format: native
output_1:
  format: %s
  size: [40, 20]
  fit: letterbox
"""

# setter -> (the value the handle holds, another valid value, a refused value); load_params takes the texts of three files
CASES = {
    "set_output_format": (("rgb_chw_f32",), ("bgr_chw_f16",), ("nope",)),
    "set_output_yuv_matrix": (("bt601",), ("bt709",), ("bt2020",)),
    "set_output_normalization": ((255.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), (1.0, (0.5, 0.25, 0.125), (2.0, 0.5, 1.5)), (0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))),
    "set_output_size": ((40, 20), (20, 30), (-1, 5)),
    "set_output_interpolation": (("linear",), ("area",), ("nearest",)),
    "set_output_roi": ((0, 0, 0, 0), (8, 4, 32, 24), (-1, 0, 4, 4)),
    "set_output_fit": (("letterbox",), ("crop",), ("fill",)),
    "set_output_pad": ((114, 114, 114), (0, 0, 0), (256, 0, 0)),
    "set_output_heads": ((2,), (3,), (0,)),
    "load_params": (PARAMS % "rgb_chw_f32", PARAMS % "bgr_chw_f16", PARAMS % "nope"),
}

# setter -> after each of the four deliveries (at the start, behind the same value, behind the other value, behind the refused
# call), for head 0 and head 1: the growth of (table builds, builds of the geometry's mask, builds of the head's delivered mask)
EXPECTED = {
    "load_params": [[(0, 1, 1), (2, 1, 1)], [(0, 1, 1), (1, 1, 1)], [(0, 0, 1), (1, 0, 1)], [(0, 0, 0), (0, 0, 0)]],
    "set_output_fit": [[(0, 1, 1), (2, 1, 1)], [(0, 0, 0), (0, 0, 1)], [(0, 0, 0), (1, 0, 1)], [(0, 0, 0), (0, 0, 1)]],
    "set_output_format": [[(0, 1, 1), (2, 1, 1)], [(0, 0, 0), (0, 0, 1)], [(0, 0, 0), (1, 0, 1)], [(0, 0, 0), (0, 0, 1)]],
    "set_output_heads": [[(0, 1, 1), (2, 1, 1)], [(0, 0, 0), (0, 0, 0)], [(0, 0, 0), (0, 0, 0)], [(0, 0, 0), (0, 0, 0)]],
    "set_output_interpolation": [[(0, 1, 1), (2, 1, 1)], [(0, 0, 0), (0, 0, 1)], [(0, 0, 0), (1, 0, 1)], [(0, 0, 0), (0, 0, 1)]],
    "set_output_normalization": [[(0, 1, 1), (2, 1, 1)], [(0, 0, 0), (1, 0, 1)], [(0, 0, 0), (1, 0, 1)], [(0, 0, 0), (0, 0, 1)]],
    "set_output_pad": [[(0, 1, 1), (2, 1, 1)], [(0, 0, 0), (0, 0, 1)], [(0, 0, 0), (0, 0, 1)], [(0, 0, 0), (0, 0, 1)]],
    "set_output_roi": [[(0, 1, 1), (2, 1, 1)], [(0, 0, 0), (0, 0, 1)], [(0, 0, 0), (1, 0, 1)], [(0, 0, 0), (0, 0, 1)]],
    "set_output_size": [[(0, 1, 1), (2, 1, 1)], [(0, 0, 0), (0, 0, 1)], [(0, 0, 0), (1, 0, 1)], [(0, 0, 0), (0, 0, 1)]],
    "set_output_yuv_matrix": [[(0, 1, 1), (2, 1, 1)], [(0, 0, 0), (0, 0, 0)], [(0, 0, 0), (0, 0, 0)], [(0, 0, 0), (0, 0, 0)]],
}


def make_pipe():
    p = RawImagePipeline(False, "", "", "", device=0)
    configure(p, cfg(undistort=True, cam=synth.camera_model(W, H)))
    p.set_undistortion_image_size(W, H)
    p.set_output_heads(2)
    p.set_rect_mask("coverage")
    p.select_output_head(1)
    p.set_output_format("rgb_chw_f32")
    p.set_output_size(40, 20)
    p.set_output_fit("letterbox")
    return p


@pytest.fixture(scope="module")
def frames():
    import torch
    return torch.from_numpy(synth.gen_frame(W, H, ENC, seed=3)[None]).cuda()


def deliver_and_count(p, frames, before):
    """One frame to both heads, the delivered mask of both; the counters of both heads, and their growth since `before`."""
    import torch
    p.apply_device_heads(frames, ENC)
    torch.cuda.synchronize()
    selected = p.get_selected_output_head()
    for k in range(2):
        p.select_output_head(k)
        p.get_output_mask(H, W, 1, ENC)
    p.select_output_head(selected)
    now = [(p.debug_output_head_info(k)[0],) + p.debug_rect_mask_info(k) for k in range(2)]
    return now, [tuple(int(a - b) for a, b in zip(n, o)) for n, o in zip(now, before)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_setting_change_rebuilds_what_it_did_before(name, frames, tmp_path):
    p = make_pipe()
    if name == "load_params":
        values = []
        for i, text in enumerate(CASES[name]):
            path = tmp_path / ("params_%d.yaml" % i)
            path.write_text(text)
            values.append((str(path),))
    else:
        values = CASES[name]
    counts, grown = deliver_and_count(p, frames, [(0, 0, 0), (0, 0, 0)])
    seen = [grown]
    for step, args in enumerate(values):
        if step < 2:
            getattr(p, name)(*args)
        else:
            with pytest.raises(ValueError):
                getattr(p, name)(*args)
        counts, grown = deliver_and_count(p, frames, counts)
        seen.append(grown)
    print('    "%s": %r,' % (name, seen))
    assert seen == EXPECTED.get(name), name
