#!/usr/bin/env python3
"""Probe: the output stage (rip_set_output_format, csrc/rip_output.hip) on config 2's geometry -- 2448 x 2048, 256 resident
frames, full chain with undistortion -- against what a PyTorch consumer does today with the native result.

Legs, all in ONE process on the same seeded frames, HIP events around whole steps, warm-up excluded, median of the rounds:
  native        the step as it is without the output stage (interleaved bgr8 out)
  rgb_chw_f16   the same step delivering normalised planar float16 / float32: one launch of output_convert_kernel more.  The
  rgb_chw_f32   converter's own time is the DIFFERENCE to the native step (the same kernels run in front of it; the last of
                them writes a 16-byte-pitched staging image instead of the caller's tensor), not a kernel timing.
  torch         out.permute(0, 3, 1, 2).flip(1).float().div(255).sub(mean).div(std) on the native result (float32 out; and
                .half() behind it for the float16 consumer): four or five passes with a temporary each.
Beside them rip_debug_hbm_probe's EXPAND13_COALESCED_NT figure of the same process -- a 1 : 3 expansion with 16-byte lanes,
the closest store shape the library measures -- and the converter's bytes per second: 3 B/px read + 3 x element B/px written.
Usage: output_format_probe.py [--frames N] [--steps K] [--rounds R] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from raw_image_pipeline_amd import RawImagePipeline  # noqa: E402

W, H = 2448, 2048
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def timed(fn, steps, rounds):
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
    return round(statistics.median(per), 4), [round(v, 4) for v in per]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    n = a.frames
    dev = torch.from_numpy(bench.make_frames(W, H, "bayer_rggb8", n, 0)).cuda()
    res = {"probe": "output_format_probe", "device": torch.cuda.get_device_name(0), "frames": n, "width": W, "height": H,
           "steps": a.steps, "rounds": a.rounds, "steps_ms": {}, "rounds_ms": {}}

    def leg(name, fn):
        res["steps_ms"][name], res["rounds_ms"][name] = timed(fn, a.steps, a.rounds)

    pipe = RawImagePipeline(False, "", "", "", device=0)
    bench.configure(pipe, "config2", W, H)
    r, c, k, _ = pipe.query_output(H, W, 1, "bayer_rggb8")
    px = n * r * c
    native = torch.empty((n, r, c, k), dtype=torch.uint8, device="cuda")
    leg("native", lambda: pipe.apply_device(dev, "bayer_rggb8", out=native))
    pipe.set_output_normalization(255.0, MEAN, STD)
    for fmt, dtype in (("rgb_chw_f16", torch.float16), ("rgb_chw_f32", torch.float32)):
        pipe.set_output_format(fmt)
        out = torch.empty((n, 3, r, c), dtype=dtype, device="cuda")
        leg(fmt, lambda: pipe.apply_device(dev, "bayer_rggb8", out=out))
        del out
    pipe.set_output_format("native")
    leg("native_again", lambda: pipe.apply_device(dev, "bayer_rggb8", out=native))
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    leg("torch_f32", lambda: native.permute(0, 3, 1, 2).flip(1).float().div(255).sub(mean).div(std))
    leg("torch_f16", lambda: native.permute(0, 3, 1, 2).flip(1).float().div(255).sub(mean).div(std).half())
    torch.cuda.empty_cache()
    res["hbm_probe_expand13_coalesced_nt_gbps"] = round(pipe.hbm_probe("expand13_coalesced_nt", 1 << 30, 10), 1)
    base = min(res["steps_ms"]["native"], res["steps_ms"]["native_again"])
    res["converter"] = {}
    for fmt, elem in (("rgb_chw_f16", 2), ("rgb_chw_f32", 4)):
        ms = round(res["steps_ms"][fmt] - base, 4)
        moved = px * (3 + 3 * elem)
        torch_ms = res["steps_ms"]["torch_f16" if elem == 2 else "torch_f32"]
        res["converter"][fmt] = {"ms_difference_to_native": ms, "bytes_moved": moved, "gbps": round(moved / (ms * 1e-3) / 1e9, 1) if ms > 0 else None,
                                 "torch_ms": torch_ms, "torch_over_converter": round(torch_ms / ms, 2) if ms > 0 else None}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
