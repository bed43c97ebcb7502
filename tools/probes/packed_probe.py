#!/usr/bin/env python3
"""Probe: packed 10- / 12-bit Bayer frames (rip_packed.hip) on 256 resident 2448 x 2048 frames, against the 16-bit pre-pass
(raw16_tile_kernel) of the parent commit's library on the same samples as uint16.

Legs, all in ONE process (both libraries live in it at once: a handle keeps the library it was created with), every other
stage off, range (64, 1023) for the 10-bit layouts and (256, 4095) for the 12-bit ones:
  parent16   the library named by --parent, bayer_rggb16 with the range: "bilinear" and "mht", flips 0 / 180 / 90
  new16      this build, the same call: the no-regression leg (bar: 1.03 x parent16)
  packed     this build, bayer_rggb{10p,12p,10_csi2,12_csi2} holding the same samples (bar: 1.25 x parent16, per kernel)
  host       submit / collect at ring depth 3 and serial apply, per frame, bayer_rggb12p against bayer_rggb16, and a vectorised
             numpy unpack of one such frame on this CPU for context
HIP events give whole steps (the pre-pass and the copy of its image into the result, which is the 8-bit chain's); the per-kernel
times the bars are about come from running this script under `rocprofv3 --kernel-trace --stats` (tools/rocpd_summary.py turns the
database into profiles/packed_kernel_stats.txt): the kernels' names carry the staging, the method and the flip.
Usage: packed_probe.py [--parent FILE.so] [--frames N] [--steps K] [--out FILE.json] [--no-host]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import raw_image_pipeline_amd.pipeline as P  # noqa: E402

W, H = 2448, 2048
RANGES = {10: (64, 1023), 12: (256, 4095)}
LAYOUTS = {"10p": 10, "12p": 12, "10_csi2": 10, "12_csi2": 12}
UNIQUE = 16   # distinct frames; the resident batch repeats them


def pack(f, layout):
    """[n, rows, cols] uint16 below 2^B -> [n, rows, row bytes] uint8 (cols % 4 == 0), group by group."""
    f = f.astype(np.uint32)
    n, rows, cols = f.shape
    if layout == "12p":
        a, b = f[..., 0::2], f[..., 1::2]
        out = np.stack([a & 255, (a >> 8) | (b & 15) << 4, b >> 4], axis=-1)
    elif layout == "12_csi2":
        a, b = f[..., 0::2], f[..., 1::2]
        out = np.stack([a >> 4, b >> 4, (a & 15) | (b & 15) << 4], axis=-1)
    elif layout == "10_csi2":
        s = [f[..., j::4] for j in range(4)]
        out = np.stack([s[0] >> 2, s[1] >> 2, s[2] >> 2, s[3] >> 2, (s[0] & 3) | (s[1] & 3) << 2 | (s[2] & 3) << 4 | (s[3] & 3) << 6], axis=-1)
    else:
        s = [f[..., j::4].astype(np.uint64) for j in range(4)]
        v = s[0] | s[1] << 10 | s[2] << 20 | s[3] << 30
        out = np.stack([(v >> (8 * k)) & 255 for k in range(5)], axis=-1)
    return out.astype(np.uint8).reshape(n, rows, -1)


def unpack12p(b, cols):
    """The CPU unpack a caller needs today in front of bayer_*16 (vectorised numpy, one thread)."""
    g = b.reshape(b.shape[0], cols // 2, 3).astype(np.uint16)
    out = np.empty((b.shape[0], cols), np.uint16)
    out[:, 0::2] = g[:, :, 0] | (g[:, :, 1] & 15) << 8
    out[:, 1::2] = g[:, :, 1] >> 4 | g[:, :, 2] << 4
    return out


def handle(library=None):
    """A handle of the given build (None: this tree's), every optional stage off."""
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


def apply_rows(pipe, frames_u8, encoding, out, n):
    """rip_apply_device on [n, H, row bytes] uint8 rows through the C interface (the parent's Python layer knows no width)."""
    rb = frames_u8.shape[2]
    pipe._call("rip_apply_device", C.c_void_p(frames_u8.data_ptr()), C.c_size_t(rb), C.c_size_t(rb * H), n, H, W, 1, encoding.encode(),
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


def host_leg(pipe, frames, encoding, n, **kw):
    """Per-frame milliseconds of a serial apply and of submit / collect with the ring kept full (depth 3)."""
    pipe.set_ring_depth(3)
    for f in frames[:3]:
        pipe.process(f, encoding, **kw)
    t0 = time.perf_counter()
    for i in range(n):
        pipe.process(frames[i % len(frames)], encoding, **kw)
    serial = (time.perf_counter() - t0) / n * 1e3
    tickets = []
    for i in range(n + 6):
        if i == 6:
            t0 = time.perf_counter()
        tickets.append(pipe.submit(frames[i % len(frames)], encoding, **kw))
        if len(tickets) == 3:
            pipe.collect(tickets.pop(0), copy=False)
    while tickets:
        pipe.collect(tickets.pop(0), copy=False)
    return round(serial, 4), round((time.perf_counter() - t0) / n * 1e3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    n = a.frames
    reps = -(-n // UNIQUE)
    f8 = bench.make_frames(W, H, "bayer_rggb8", min(n, UNIQUE), 0)
    samples = {10: (64 + f8.astype(np.uint16) * 4).clip(0, 1023).astype(np.uint16),     # a little beyond the white level
               12: (256 + f8.astype(np.uint16) * 16).clip(0, 4095).astype(np.uint16)}
    del f8
    res = {"probe": "packed_probe", "device": torch.cuda.get_device_name(0), "frames": n, "width": W, "height": H,
           "ranges": {str(k): list(v) for k, v in RANGES.items()}, "steps_ms": {}, "host_ms_per_frame": {}}
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
    new = handle()
    new.set_debayer_16bit(True)
    old = handle(a.parent) if a.parent else None
    if old is not None:
        old.set_debayer_16bit(True)

    def resident(host):
        return torch.from_numpy(host).cuda().repeat(reps, 1, 1)[:n].contiguous()

    for bits in (10, 12):
        dev16 = resident(samples[bits].view(np.uint8).reshape(-1, H, W * 2))
        packed = {layout: resident(pack(samples[bits], layout)) for layout, b in LAYOUTS.items() if b == bits}
        for p in (new, old):
            if p is not None:
                p.set_debayer_16bit_range(*RANGES[bits])
        for angle in (0, 180, 90):
            for p in (new, old):
                if p is not None:
                    p.set_flip(angle != 0)
                    p.set_flip_angle(angle)
            for method in ("bilinear", "mht"):
                for p in (new, old):
                    if p is not None:
                        p.set_debayer_method(method)
                key = "%dbit_%s_flip%d" % (bits, method, angle)
                # the yardstick before and after the legs it is compared with
                if old is not None:
                    res["steps_ms"]["parent16_" + key] = timed(lambda: apply_rows(old, dev16, "bayer_rggb16", out, n), a.steps)
                res["steps_ms"]["new16_" + key] = timed(lambda: apply_rows(new, dev16, "bayer_rggb16", out, n), a.steps)
                for layout, dev in packed.items():
                    res["steps_ms"]["%s_%s_flip%d" % (layout, method, angle)] = timed(lambda: apply_rows(new, dev, "bayer_rggb" + layout, out, n), a.steps)
                if old is not None:
                    res["steps_ms"]["parent16_" + key + "_again"] = timed(lambda: apply_rows(old, dev16, "bayer_rggb16", out, n), a.steps)
        del dev16, packed
    del out
    if not a.no_host:
        for p in (new,):
            p.set_flip(False)
            p.set_debayer_method("bilinear")
            p.set_debayer_16bit_range(*RANGES[12])
        f16 = [np.ascontiguousarray(f) for f in samples[12][:8]]
        f12 = [np.ascontiguousarray(f) for f in pack(samples[12][:8], "12p")]
        serial, ring = host_leg(new, f16, "bayer_rggb16", 60)
        res["host_ms_per_frame"]["bayer_rggb16"] = {"serial_apply": serial, "submit_collect_depth3": ring, "upload_bytes": int(f16[0].nbytes)}
        serial, ring = host_leg(new, f12, "bayer_rggb12p", 60)
        res["host_ms_per_frame"]["bayer_rggb12p"] = {"serial_apply": serial, "submit_collect_depth3": ring, "upload_bytes": int(f12[0].nbytes)}
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            u = unpack12p(f12[0], W)
            t.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(u, f16[0])
        res["host_ms_per_frame"]["numpy_unpack_12p_on_this_cpu"] = round(min(t), 3)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
