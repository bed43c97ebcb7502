"""Head sets for the output heads (include/rip.h rip_set_output_heads): which frames, which pipeline settings and which heads the
tests of tests/test_heads.py (CPU: queries under every selection against a twin handle) and tests/test_heads_gpu.py (every delivered
byte against a twin handle whose only output is that head) run.  The expectation is always the single-output path on a twin; nothing
here needs an oracle.

Frames (width x height; the names of PARITY.md "Variant coverage"): 136 x 72 Bayer without undistortion -- 408 bytes per row of F, no
multiple of 16, so a tight identity head is copied; 200 x 136 with undistortion (600 bytes, copied) and 208 x 136 (624 = 39 x 16 bytes:
a tight identity head is written directly); one mono8 frame of 65 x 33.

Importable without a GPU; nothing here looks at the library."""
import collections

import helpers as H
from raw_image_pipeline_amd import synth

Head = collections.namedtuple("Head", ["format", "norm", "size", "interp", "roi", "fit", "pad"])
Head.__new__.__defaults__ = ("native", (255.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), (0, 0), "linear", (0, 0, 0, 0), "stretch", (114, 114, 114))
DEFAULT = Head()

IDENTITY = Head()
# 64 x 48 letterbox area rgb_chw_f16 with a non-trivial normalisation
LETTERBOX_F16 = Head(format="rgb_chw_f16", norm=(57.0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), size=(64, 48), interp="area", fit="letterbox",
                     pad=(3, 128, 250))
CROP_CUBIC = Head(format="rgb8", size=(96, 64), interp="cubic_aa", fit="crop")
WINDOW_MONO = Head(format="mono8", roi=(8, 4, 64, 32))          # a window without a target
UPSCALE = Head(size=(300, 100), interp="linear")                  # native, written into the caller's buffer by the resize
AA_BF16 = Head(format="bgr_chw_bf16", norm=(255.0, (0.5, 0.25, 0.125), (2.0, 0.5, 1.5)), size=(50, 40), interp="linear_aa")


def mean2(frame):
    """The exact 2 x 2 mean under "area" for a frame's F: half of each side."""
    w, h = FRAMES[frame].f_size
    return Head(format="bgr_chw_f32", size=(w // 2, h // 2), interp="area")


Frame = collections.namedtuple("Frame", ["size", "encoding", "channels", "f_size", "cfg"])
FRAMES = {
    "bayer136": Frame((136, 72), "bayer_rggb8", 1, (136, 72), dict(wb=True, wb_method="grey_world", cc=True, gamma=True)),
    "und200": Frame((200, 136), "bayer_rggb8", 1, (200, 136), dict(wb=True, wb_method="grey_world", gamma=True, undistort=True)),
    "und208": Frame((208, 136), "bayer_grbg8", 1, (208, 136), dict(gamma=True, flip=True, flip_angle=180, undistort=True)),
    "mono65": Frame((65, 33), "mono8", 1, (65, 33), dict(gamma=True)),
}

HeadSet = collections.namedtuple("HeadSet", ["name", "frame", "heads"])
SETS = [
    HeadSet("identity_and_tensor", "bayer136", (IDENTITY, LETTERBOX_F16)),
    HeadSet("two_identities_direct", "und208", (IDENTITY, IDENTITY, CROP_CUBIC)),
    HeadSet("no_identity", "bayer136", (LETTERBOX_F16, CROP_CUBIC, WINDOW_MONO)),
    HeadSet("mean_upscale_aa", "und200", (IDENTITY, mean2("und200"), UPSCALE, AA_BF16)),
    HeadSet("one_channel", "mono65", (IDENTITY, Head(format="mono8", roi=(8, 4, 32, 16)), Head(size=(40, 20)), Head(size=(30, 15), interp="area"))),
    HeadSet("eight", "und208", (LETTERBOX_F16, IDENTITY, CROP_CUBIC, WINDOW_MONO, mean2("und208"), UPSCALE, AA_BF16, IDENTITY)),
]
BY_NAME = {s.name: s for s in SETS}
assert len(BY_NAME) == len(SETS)


def set_id(s):
    return s.name


def frame_cfg(frame):
    """helpers.cfg of a frame's pipeline settings (the camera of the frames with undistortion included)."""
    f = FRAMES[frame]
    c = dict(f.cfg)
    if c.get("undistort"):
        c["cam"] = synth.camera_model(*f.size)
    return H.cfg(**c)


def configure_pipeline(pipe, frame):
    H.configure(pipe, frame_cfg(frame))


def apply_head(pipe, head):
    """The settings of `head` through the single-output setters: they go to the selected head."""
    pipe.set_output_format(head.format)
    pipe.set_output_normalization(*head.norm)
    pipe.set_output_size(*head.size)
    pipe.set_output_interpolation(head.interp)
    pipe.set_output_roi(*head.roi)
    pipe.set_output_fit(head.fit)
    pipe.set_output_pad(*head.pad)


def read_head(pipe):
    """The selected head's settings as a Head."""
    return Head(pipe.get_output_format(), pipe.get_output_normalization(), pipe.get_output_size(), pipe.get_output_interpolation(),
                pipe.get_output_roi(), pipe.get_output_fit(), pipe.get_output_pad())


def configure_heads(pipe, heads):
    pipe.set_output_heads(len(heads))
    for k, h in enumerate(heads):
        pipe.select_output_head(k)
        apply_head(pipe, h)
    pipe.select_output_head(0)


def gen_frames(frame, n, seed=0):
    """n host frames of a FRAMES entry, [n, rows, cols] uint8."""
    import numpy as np
    f = FRAMES[frame]
    w, h = f.size
    if f.encoding == "mono8":
        return np.stack([synth.gen_scene_bgr(w, h, seed + i)[..., 1].copy() for i in range(n)])
    return np.stack([synth.gen_frame(w, h, f.encoding, seed=seed + i) for i in range(n)])
