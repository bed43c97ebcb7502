#!/usr/bin/env python3
"""Probe: what the Malvar-He-Cutler demosaic (rip_set_debayer_method "mht") costs against the bilinear one, in one process on
the same seeded frames, the two methods alternated on one handle per leg (HIP events around apply_device after a warm-up;
median of the rounds).  Legs:
  demosaic   2448x2048 bayer_rggb8, 256 frames, nothing but the demosaic, flip 0 and flip 90
  config2    the BASELINE config-2 stage set (bench.py configure "config2") through apply_device, 256 frames
  config5    debayer + undistortion at 3840x2160, 64 frames (config 5's per-GPU share of a 512-frame batch)
Per class (rip_profile_*): the MHT pass counts as "chain", so on the demosaic leg "chain" holds the MHT kernel AND the copy the
chain makes of its image; the per-kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of this script.
Usage: debayer_method_probe.py [--out FILE.json] [--rounds R] [--steps K] [--legs demosaic,config2,config5]"""
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

METHODS = ("bilinear", "mht")


def time_steps(pipe, frames, pattern, out, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        pipe.apply_device(frames, pattern, out=out)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def class_times(pipe, frames, pattern, out):
    pipe.profile_begin(64)
    pipe.apply_device(frames, pattern, out=out)
    res = pipe.profile_end()
    return {k: {"ms": round(ms, 4), "launches": n} for k, (ms, n) in res.items() if n}


def leg(name, width, height, n, setup, rounds, steps):
    frames = torch.from_numpy(bench.make_frames(width, height, "bayer_rggb8", n, 0)).cuda()
    pipe = RawImagePipeline(False, "", "", "", device=0)
    pattern, stages = setup(pipe)
    r, c, k, _ = pipe.query_output(height, width, 1, pattern)
    out = torch.empty((n, r, c, k), dtype=torch.uint8, device="cuda")
    per = {m: [] for m in METHODS}
    classes = {}
    for _ in range(rounds):
        for m in METHODS:
            pipe.set_debayer_method(m)
            pipe.apply_device(frames, pattern, out=out)  # warm-up: buffers, tables, plan
            torch.cuda.synchronize()
            per[m].append(time_steps(pipe, frames, pattern, out, steps))
            classes[m] = class_times(pipe, frames, pattern, out)
    res = {"leg": name, "stages": stages, "frames": n, "width": width, "height": height, "rounds": rounds, "steps": steps}
    for m in METHODS:
        med = statistics.median(per[m])
        res[m] = {"ms_per_step": round(med, 4), "rounds_ms": [round(v, 4) for v in per[m]],
                  "frames_per_s": round(n * 1000.0 / med, 1), "classes": classes[m]}
    res["mht_over_bilinear"] = round(res["mht"]["ms_per_step"] / res["bilinear"]["ms_per_step"], 4)
    print(json.dumps(res), flush=True)
    return res


def demosaic_only(angle):
    def setup(pipe):
        for f in (pipe.set_white_balance, pipe.set_color_calibration, pipe.set_gamma_correction, pipe.set_vignetting_correction,
                  pipe.set_color_enhancer, pipe.set_undistortion):
            f(False)
        pipe.set_flip(angle != 0)
        pipe.set_flip_angle(angle)
        return "bayer_rggb8", "debayer" + ("+flip%d" % angle if angle else "")
    return setup


def bench_workload(workload, width, height):
    def setup(pipe):
        return bench.configure(pipe, workload, width, height)
    return setup


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--legs", default="demosaic,config2,config5")
    a = ap.parse_args()
    legs = a.legs.split(",")
    results = []
    if "demosaic" in legs:
        for angle in (0, 90):
            results.append(leg("demosaic_flip%d" % angle, 2448, 2048, 256, demosaic_only(angle), a.rounds, a.steps))
    if "config2" in legs:
        results.append(leg("config2", 2448, 2048, 256, bench_workload("config2", 2448, 2048), a.rounds, a.steps))
    if "config5" in legs:
        results.append(leg("config5", 3840, 2160, 64, bench_workload("config5", 3840, 2160), a.rounds, a.steps))
    doc = {"probe": "debayer_method_probe", "device": torch.cuda.get_device_name(0), "results": results}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
