#!/usr/bin/env python3
"""Probe: the 16-bit pre-pass (rip_raw16.hip: demosaic at 16 bits + narrowing + flip) on 256 resident 2448 x 2048 frames.

Legs, all in ONE process on the same seeded uint16 frames:
  raw16      this build, rip_set_debayer_16bit_range(64, 1023), every other stage off: "bilinear" and "mht", flips 0 / 180 / 90.
             2 B/px read + 3 B/px written by raw16_tile_kernel (the copy of its image into the result that follows is the
             8-bit chain's, not the pre-pass).
  yardstick  the library named by --parent (a build of the parent commit), range off: debayer16_kernel, 2 B/px read + 6 B/px
             written (bgr16), same API call.  Skipped without --parent.
  config2    for context: config 2's stage set end to end on bayer_rggb16 frames with the range against bayer_rggb8 frames.
HIP events give whole steps; the per-kernel split comes from running this script under `rocprofv3 --kernel-trace --stats`
(tools/rocpd_summary.py turns the database into profiles/raw16_kernel_stats.txt).  Both libraries live in the process at once:
a handle keeps the library it was created with.
Usage: raw16_probe.py [--parent FILE.so] [--frames N] [--steps K] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import raw_image_pipeline_amd.pipeline as P  # noqa: E402

W, H = 2448, 2048
BLACK, WHITE = 64, 1023


def handle(library=None):
    """A handle of the given build (None: this tree's)."""
    P._lib = None  # load_library caches one library per process; every handle keeps the one it was created with
    if library:
        os.environ["RIP_LIBRARY"] = os.path.abspath(library)
    else:
        os.environ.pop("RIP_LIBRARY", None)
    pipe = P.RawImagePipeline(False, "", "", "", device=0)
    os.environ.pop("RIP_LIBRARY", None)
    P._lib = None
    for f in (pipe.set_white_balance, pipe.set_color_calibration, pipe.set_gamma_correction, pipe.set_vignetting_correction,
              pipe.set_color_enhancer, pipe.set_undistortion):
        f(False)
    return pipe


def apply16(pipe, frames_u8, out, n):
    """rip_apply_device on the byte view of uint16 frames, through the C interface (the parent's Python layer has no 16-bit batch)."""
    pipe._call("rip_apply_device", C.c_void_p(frames_u8.data_ptr()), C.c_size_t(W * 2), C.c_size_t(W * 2 * H), n, H, W, 1, b"bayer_rggb16",
               C.c_void_p(out.data_ptr()), C.c_size_t(0), C.c_size_t(0), None, None)


def timed(fn, steps, rounds=3):
    per = []
    for _ in range(rounds):
        fn()
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(steps):
            fn()
        end.record()
        torch.cuda.synchronize()
        per.append(start.elapsed_time(end) / steps)
    return round(statistics.median(per), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = a.frames
    f8 = bench.make_frames(W, H, "bayer_rggb8", n, 0)
    # 10-bit data with a black level of 64, a little beyond the white level in the highlights
    f16 = (BLACK + f8.astype(np.uint16) * 4).astype(np.uint16)
    dev8 = torch.from_numpy(f8).cuda()
    dev16 = torch.from_numpy(f16.view(np.uint8).reshape(n, H, W * 2)).cuda()
    del f8, f16
    res = {"probe": "raw16_probe", "device": torch.cuda.get_device_name(0), "frames": n, "width": W, "height": H, "range": [BLACK, WHITE], "steps_ms": {}}
    out8 = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
    new = handle()
    new.set_debayer_16bit(True)
    old = handle(a.parent) if a.parent else None
    if old is not None:
        old.set_debayer_16bit(True)
        out16 = torch.empty((n, H, W, 6), dtype=torch.uint8, device="cuda")
    for angle in (0, 180, 90):
        for p in (new, old):
            if p is not None:
                p.set_flip(angle != 0)
                p.set_flip_angle(angle)
        # alternate the two builds
        if old is not None:
            old.set_debayer_method("bilinear")
            res["steps_ms"]["parent_bgr16_bilinear_flip%d" % angle] = timed(lambda: apply16(old, dev16, out16, n), a.steps)
        for method in ("bilinear", "mht"):
            new.set_debayer_method(method)
            new.set_debayer_16bit_range(BLACK, WHITE)
            res["steps_ms"]["raw16_%s_flip%d" % (method, angle)] = timed(lambda: apply16(new, dev16, out8, n), a.steps)
        if old is not None:
            res["steps_ms"]["parent_bgr16_bilinear_flip%d_again" % angle] = timed(lambda: apply16(old, dev16, out16, n), a.steps)
    if old is not None:
        del out16
    # context: config 2 end to end, 16-bit frames with the range against 8-bit frames, same build
    for enc in ("bayer_rggb8", "bayer_rggb16"):
        pipe = handle()
        bench.configure(pipe, "config2", W, H)
        pipe.set_debayer_16bit(True)
        pipe.set_debayer_16bit_range(BLACK, WHITE)
        r, c, k, _ = pipe.query_output(H, W, 1, enc)
        out = torch.empty((n, r, c, k), dtype=torch.uint8, device="cuda")
        frames = dev16 if enc.endswith("16") else dev8
        res["steps_ms"]["config2_" + enc] = timed(lambda: pipe.apply_device(frames, enc, out=out), a.steps)
        del out
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
