#!/usr/bin/env python3
"""Probe: output heads (rip_apply_device_heads) on 64 resident 2448 x 2048 bayer_rggb8 frames under config 2's settings, against the
parent commit's library delivering the same products.  Heads: {identity bgr8, tightly packed; 640 x 480 letterbox area rgb_chw_f16}.

Legs, all in ONE process (both libraries live in it at once: a handle keeps the library it was created with):
  a  the library named by --parent delivering the tensor alone (one handle, rip_apply_device)
  b  that library on two handles delivering both products (the whole chain twice)
  c  this build's heads call; the identity head is 16-byte aligned, so the chain writes it directly
  d  c with the identity head's base 4 bytes in: F goes to the staging image and head_copy_kernel delivers the head
  e  head_copy_kernel alone (launch_head_copy of librip_heads_hip.so called directly), with its bytes per second
HIP events on the handle's stream around every step, warm-up excluded, median of 10.  Bar: c <= 1.05 x a (with the direct write c
launches the kernels a launches).  No bar on d and e: they are reported beside b and beside rip_probe.hip's streaming-copy rate.
Usage: heads_probe.py [--parent FILE.so] [--frames N] [--steps K] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import raw_image_pipeline_amd.pipeline as P  # noqa: E402
from raw_image_pipeline_amd import build as B  # noqa: E402

W, H = 2448, 2048
TENSOR = dict(format="rgb_chw_f16", size=(640, 480), interp="area", fit="letterbox")
UNIQUE = 16   # distinct frames; the resident batch repeats them


def handle(library=None):
    """A handle of the given build (None: this tree's) under config 2's settings."""
    P._lib = None  # load_library caches one library per process; every handle keeps the one it was created with
    if library:
        os.environ["RIP_LIBRARY"] = os.path.abspath(library)
    else:
        os.environ.pop("RIP_LIBRARY", None)
    pipe = P.RawImagePipeline(False, "", "", "", device=0)
    os.environ.pop("RIP_LIBRARY", None)
    P._lib = None
    bench.configure(pipe, "config2", W, H)
    return pipe


def tensor_output(pipe):
    """The tensor's settings through the single-output setters (they go to the selected head)."""
    pipe._call("rip_set_output_format", TENSOR["format"].encode())
    pipe._call("rip_set_output_size", *TENSOR["size"])
    pipe._call("rip_set_output_interpolation", TENSOR["interp"].encode())
    pipe._call("rip_set_output_fit", TENSOR["fit"].encode())


def single(pipe, frames, out):
    pipe._call("rip_apply_device", C.c_void_p(frames.data_ptr()), C.c_size_t(0), C.c_size_t(0), frames.shape[0], H, W, 1, b"bayer_rggb8",
               C.c_void_p(out.data_ptr()), C.c_size_t(0), C.c_size_t(0), None, None)


def heads(pipe, frames, image_ptr, tensor):
    bufs = (P._HeadBuffer * 2)(P._HeadBuffer(C.c_void_p(image_ptr), 0, 0), P._HeadBuffer(C.c_void_p(tensor.data_ptr()), 0, 0))
    pipe._call("rip_apply_device_heads", C.c_void_p(frames.data_ptr()), C.c_size_t(0), C.c_size_t(0), frames.shape[0], H, W, 1, b"bayer_rggb8",
               bufs, 2, None, None)


class HeadCopyParams(C.Structure):
    """rip::HeadCopyParams (csrc/rip_heads.hpp)."""
    _fields_ = [("src", C.c_void_p), ("src_step", C.c_size_t), ("src_frame_stride", C.c_size_t), ("dst", C.c_void_p), ("dst_step", C.c_size_t),
                ("dst_frame_stride", C.c_size_t), ("rows", C.c_int), ("n_frames", C.c_int), ("row_bytes", C.c_size_t)]


def timed(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(steps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        per.append(start.elapsed_time(end))
    return {"median_ms": round(statistics.median(per), 4), "min_ms": round(min(per), 4), "max_ms": round(max(per), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = a.frames
    host = bench.make_frames(W, H, "bayer_rggb8", min(n, UNIQUE), 0)
    frames = torch.from_numpy(host).cuda().repeat(-(-n // UNIQUE), 1, 1)[:n].contiguous()
    row = W * 3
    backing = torch.empty(n * H * row + 16, dtype=torch.uint8, device="cuda")   # the identity head: tight, at a 16-byte aligned base or 4 bytes in
    assert backing.data_ptr() % 16 == 0 and row % 16 == 0
    image = backing[:n * H * row].view(n, H, W, 3)
    shifted = backing[4:4 + n * H * row].view(n, H, W, 3)
    tensor = torch.empty((n, 3, TENSOR["size"][1], TENSOR["size"][0]), dtype=torch.float16, device="cuda")
    res = {"probe": "heads_probe", "device": torch.cuda.get_device_name(0), "frames": n, "width": W, "height": H, "steps": a.steps,
           "heads": ["identity bgr8 tight", "640x480 letterbox area rgb_chw_f16"], "ms": {}}

    new = handle()
    new._call("rip_set_output_heads", 2)
    new._call("rip_select_output_head", 1)
    tensor_output(new)
    new._call("rip_select_output_head", 0)
    old_tensor = old_image = None
    if a.parent:
        old_tensor, old_image = handle(a.parent), handle(a.parent)
        tensor_output(old_tensor)

    def leg_b():
        single(old_image, frames, image)
        single(old_tensor, frames, tensor)

    # the bytes first: both products equal the single-output calls' (of the parent where it is given, else of this build)
    ref_tensor_pipe, ref_image_pipe = (old_tensor, old_image) if a.parent else (handle(), handle())
    if not a.parent:
        tensor_output(ref_tensor_pipe)
    want_image, want_tensor = torch.empty_like(image), torch.empty_like(tensor)
    single(ref_image_pipe, frames, want_image)
    single(ref_tensor_pipe, frames, want_tensor)
    for target in (image, shifted):
        target.zero_()
        tensor.zero_()
        heads(new, frames, target.data_ptr(), tensor)
        torch.cuda.synchronize()
        assert torch.equal(target, want_image) and torch.equal(tensor.view(torch.int16), want_tensor.view(torch.int16)), "heads call differs from the single-output calls"
    del want_image, want_tensor

    if a.parent:
        res["ms"]["a_parent_tensor_alone"] = timed(lambda: single(old_tensor, frames, tensor), a.steps)
        res["ms"]["b_parent_two_handles"] = timed(leg_b, a.steps)
    res["ms"]["c_heads_direct_write"] = timed(lambda: heads(new, frames, image.data_ptr(), tensor), a.steps)
    res["direct_write_c"] = new.debug_output_head_info(0)[1:]
    res["ms"]["d_heads_copy_path"] = timed(lambda: heads(new, frames, shifted.data_ptr(), tensor), a.steps)
    res["direct_write_d"] = new.debug_output_head_info(0)[1:]
    if a.parent:
        res["ms"]["a_parent_tensor_alone_again"] = timed(lambda: single(old_tensor, frames, tensor), a.steps)
        ya = statistics.mean([res["ms"]["a_parent_tensor_alone"]["median_ms"], res["ms"]["a_parent_tensor_alone_again"]["median_ms"]])
        res["ratio_c_over_a"] = round(res["ms"]["c_heads_direct_write"]["median_ms"] / ya, 4)
        res["ratio_d_over_a"] = round(res["ms"]["d_heads_copy_path"]["median_ms"] / ya, 4)
        res["ratio_b_over_a"] = round(res["ms"]["b_parent_two_handles"]["median_ms"] / ya, 4)
        res["bar_c_at_most_1_05_a"] = res["ratio_c_over_a"] <= 1.05

    # e: the copy kernel alone, from a staging image of F's padded pitch into the shifted buffer
    lib = C.CDLL(B.kernel_library("heads").out)
    launch = getattr(lib, "_ZN3rip16launch_head_copyERKNS_14HeadCopyParamsEP12ihipStream_tPNS_10LaunchInfoE")
    launch.restype = C.c_bool
    staging = torch.empty(n * H * row, dtype=torch.uint8, device="cuda")
    prm = HeadCopyParams(staging.data_ptr(), row, row * H, shifted.data_ptr(), row, row * H, H, n, row)
    assert launch(C.byref(prm), None, None)
    res["ms"]["e_head_copy_kernel_alone"] = timed(lambda: launch(C.byref(prm), None, None), a.steps)
    res["head_copy_GBps_read_plus_written"] = round(2 * n * H * row / (res["ms"]["e_head_copy_kernel_alone"]["median_ms"] * 1e-3) / 1e9, 1)
    prm.dst = image.data_ptr()
    res["ms"]["e_head_copy_kernel_alone_aligned_dst"] = timed(lambda: launch(C.byref(prm), None, None), a.steps)
    res["streaming_copy_probe_GBps"] = round(new.hbm_probe("copy", nbytes=n * H * row, reps=10), 1)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
