#!/usr/bin/env python3
"""Counterpart of the reference's raw_image_pipeline_python/scripts/apply_pipeline.py on synthetic data:
construct the pipeline from three YAML files, print the calibration it holds, run process() (returns a
copy) and apply() (re-seats the input) on a colour image, and write both results as PNG when Pillow is
available (the reference uses cv2 / rospkg and its bundled alphasense.png, which are not shipped here).

usage: python examples/apply_pipeline.py [--device 0] [--out-dir .] [--model equidistant|plumb_bob|rational_polynomial]
"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from raw_image_pipeline_amd import RawImagePipeline, synth  # noqa: E402
from raw_image_pipeline_amd.pipeline import yuv_planes  # noqa: E402

# example coefficients of the pinhole models (k1 k2 p1 p2 k3 [k4 k5 k6])
PINHOLE_EXAMPLES = {"plumb_bob": [-0.28, 0.07, 2e-4, -3e-4, 0.0],
                    "rational_polynomial": [0.9, 0.25, 3e-4, -2e-4, 0.01, 1.25, 0.55, 0.05]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out-dir", default=".")
    ap.add_argument("--model", default="equidistant", choices=sorted(PINHOLE_EXAMPLES) + ["equidistant"],
                    help="distortion model of the synthetic calibration (the pinhole models report 5 / 8 coefficients)")
    args = ap.parse_args()

    w, h = 720, 540  # the size of the reference's example calibration
    img = synth.gen_scene_bgr(w, h, seed=7)
    tmp = tempfile.mkdtemp(prefix="rip_demo_")
    calib_file = os.path.join(tmp, "calib.yaml")
    color_calib_file = os.path.join(tmp, "color_calib.yaml")
    param_file = os.path.join(tmp, "params.yaml")
    with open(calib_file, "w") as f:
        if args.model in PINHOLE_EXAMPLES:
            f.write(synth.calibration_yaml(synth.pinhole_camera_model(w, h, PINHOLE_EXAMPLES[args.model]), args.model))
        else:
            f.write(synth.calibration_yaml(synth.camera_model(w, h)))
    with open(color_calib_file, "w") as f:
        f.write("matrix:\n  rows: 3\n  cols: 3\n  data: %s\nbias:\n  rows: 3\n  cols: 1\n  data: [0.0, 0.0, 0.0]\n" % synth.COLOR_MATRIX)
    with open(param_file, "w") as f:
        f.write("debayer:\n  enabled: true\n  encoding: \"auto\"\nflip:\n  enabled: false\n  angle: 0\n"
                "white_balance:\n  enabled: true\n  method: \"grey_world\"\n  saturation_bright_thr: 0.8\n  saturation_dark_thr: 0.2\n"
                "color_calibration:\n  enabled: false\ngamma_correction:\n  enabled: false\n  method: \"custom\"\n  k: 0.8\n"
                "vignetting_correction:\n  enabled: false\n  scale: 1.5\n  a2: 1e-3\n  a4: 1e-6\n"
                "color_enhancer:\n  hue_gain: 1.0\n  saturation_gain: 1.5\n  value_gain: 1.0\n"
                "undistortion:\n  enabled: true\n  balance: 0.0\n  fov_scale: 0.8\n")

    proc = RawImagePipeline(False, param_file, calib_file, color_calib_file, device=args.device)

    # camera-info getters of both geometries (what the ROS node copies into sensor_msgs/CameraInfo)
    fields = ("image_height", "image_width", "distortion_model", "camera_matrix", "distortion_coefficients", "rectification_matrix",
              "projection_matrix")
    for title, side in (("distorted input (dist)", "dist"), ("after undistortion (rect)", "rect")):
        print("%s:" % title)
        for name in fields:
            value = getattr(proc, "get_%s_%s" % (side, name))()
            print("  %-28s %s" % (side + "_" + name, np.array2string(np.asarray(value), precision=4, suppress_small=True)
                                   if not isinstance(value, (str, int)) else value))

    img2 = proc.process(img, "bgr8")   # returns a new image, `img` stays as it was
    before = img.copy()
    out = proc.apply(img, "bgr8")      # in place: `img` now holds the result
    assert np.array_equal(out, img2) and np.array_equal(img, out) and not np.array_equal(before, img)
    proc.set_output_size(w // 2, h // 2)  # the GPU resizes what it delivers (cv::resize, INTER_LINEAR); here the 2 x 2 mean
    print("half size:", proc.process(before, "bgr8").shape, "camera matrix:", proc.get_output_camera_info(h, w, 3, "bgr8")[2].round(3).tolist())
    proc.set_output_interpolation("area")  # cv::resize's INTER_AREA: every source pixel under an output pixel counts (downscales only)
    proc.set_output_size(w // 4, h // 3)
    print("area,", proc.get_output_interpolation() + ":", proc.process(before, "bgr8").shape)
    proc.set_output_size(w // 4, w // 4)  # a square network input: keep the aspect and pad ("letterbox"), or cut the centre ("crop")
    for fit in ("letterbox", "crop"):
        proc.set_output_fit(fit)
        read, picture = proc.get_output_window(h, w, 3, "bgr8")
        print("%s: reads %s of the image, picture at %s of %s" % (fit, read, picture, proc.process(before, "bgr8").shape))
    proc.set_output_fit("stretch")
    # for an encoder: YUV 4:2:0 in one [3 H / 2, W] buffer, half the bytes of bgr8 on the way to the host
    proc.set_output_size(w // 2, h // 2)
    proc.set_output_format("nv12")
    proc.set_output_yuv_matrix("bt709")
    nv12 = proc.process(before, "bgr8")
    y, cb, cr = yuv_planes(nv12, "nv12")
    print("nv12:", nv12.shape, "Y", y.shape, "Cb / Cr", cb.shape, "mean (Y, Cb, Cr): %.1f %.1f %.1f" % (y.mean(), cb.mean(), cr.mean()))
    # the same picture as a baseline JPEG, encoded on the GPU: process() returns the stream, trimmed to its length
    proc.set_output_format("jpeg")
    proc.set_output_jpeg(90, 1)
    stream = proc.process(before, "bgr8")
    jpg = os.path.join(args.out_dir, "apply_pipeline.jpg")
    with open(jpg, "wb") as f:
        f.write(stream.tobytes())
    print("jpeg: %d bytes (quality 90) -> %s" % (stream.size, jpg))
    proc.set_output_format("native")
    proc.set_output_size(0, 0)
    # for a visual-inertial front end: the colour image on head 0 and, from the same chain run, the equalised grey image a feature
    # tracker wants on head 1 -- cv2.createCLAHE(3.0, (8, 8)).apply(grey) restated, on the GPU
    proc.set_output_heads(2)
    proc.select_output_head(1)
    proc.set_output_format("mono8")
    proc.set_output_clahe(3.0, 8, 8)
    proc.select_output_head(0)
    colour, grey = proc.apply_heads(before, "bgr8")
    print("heads:", colour.shape, "and mono8 + CLAHE", grey.shape, "std of the grey image %.1f" % grey.std())
    proc.set_output_heads(1)
    try:
        from PIL import Image
        Image.fromarray(img[..., ::-1]).save(os.path.join(args.out_dir, "output_apply.png"))
        Image.fromarray(img2[..., ::-1]).save(os.path.join(args.out_dir, "output_process.png"))
        print("wrote output_apply.png / output_process.png")
    except ImportError:
        np.save(os.path.join(args.out_dir, "output_process.npy"), img2)
        print("Pillow not available: wrote output_process.npy")


if __name__ == "__main__":
    main()
