"""Times of the antialiased resize kernels (csrc/rip_aa.hip) beside the area kernel, launches alone on one resident batch.

64 frames of 2448 x 2048 x 3 -> 640 x 480: rip::launch_aa of librip_aa_hip.so under "linear_aa" and under "cubic_aa", and
rip::launch_area_reduce of librip_area_hip.so, called directly on host-built tables, in one process, the three legs alternating:
HIP events around 4 launches, 5 rounds per leg, after 2 warm-up launches each.  (rip_profile_begin / end times the chain's four
kernel classes; the resize stage's launches are not among them, so the events sit around the launches themselves.)  One frame of
every leg is compared with its reference first.  Every line printed is also written to the output file.
Usage: aa_probe.py [OUT.txt]   (default profiles/resize_aa_kernel_times.txt)"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from raw_image_pipeline_amd import load_library  # noqa: E402
from raw_image_pipeline_amd import build as B  # noqa: E402

N, R_, C_, H, W = 64, 2048, 2448, 480, 640
OUT = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "resize_aa_kernel_times.txt"), "w")


def say(line):
    print(line, flush=True)
    OUT.write(line + "\n")
    OUT.flush()


class AreaParams(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_step", C.c_size_t), ("src_frame_stride", C.c_size_t), ("dst", C.c_void_p), ("dst_step", C.c_size_t),
                ("dst_frame_stride", C.c_size_t), ("src_rows", C.c_int), ("src_cols", C.c_int), ("rows", C.c_int), ("cols", C.c_int),
                ("channels", C.c_int), ("n_frames", C.c_int), ("whole", C.c_int), ("scale", C.c_float), ("xfirst", C.c_void_p), ("xcount", C.c_void_p),
                ("xwofs", C.c_void_p), ("xweight", C.c_void_p), ("yfirst", C.c_void_p), ("ycount", C.c_void_p), ("ywofs", C.c_void_p), ("yweight", C.c_void_p)]


class AaParams(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_step", C.c_size_t), ("src_frame_stride", C.c_size_t), ("dst", C.c_void_p), ("dst_step", C.c_size_t),
                ("dst_frame_stride", C.c_size_t), ("src_rows", C.c_int), ("src_cols", C.c_int), ("rows", C.c_int), ("cols", C.c_int),
                ("channels", C.c_int), ("n_frames", C.c_int), ("tile_rows", C.c_int), ("lds_rows", C.c_int), ("xprec", C.c_int), ("yprec", C.c_int),
                ("xfirst", C.c_void_p), ("xcount", C.c_void_p), ("xwofs", C.c_void_p), ("xweight", C.c_void_p), ("yfirst", C.c_void_p), ("ycount", C.c_void_p),
                ("ywofs", C.c_void_p), ("yweight", C.c_void_p)]


class FitWindow(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("frame_cols", C.c_int), ("frame_rows", C.c_int)]


ptr = lambda a: a.ctypes.data_as(C.c_void_p)


def area_launch(lib, frames, dst):
    launch = getattr(C.CDLL(B.kernel_library("area").out), "_ZN3rip18launch_area_reduceERKNS_10AreaParamsEP12ihipStream_tPNS_10LaunchInfoE")
    launch.restype = C.c_bool
    xf, xc, xw = np.zeros(W, np.int32), np.zeros(W, np.int32), np.zeros(C_ + 2 * W, np.float32)
    yf, yc, yw = np.zeros(H, np.int32), np.zeros(H, np.int32), np.zeros(R_ + 2 * H, np.float32)
    whole, scale = C.c_int(0), C.c_float(0)
    assert lib.rip_debug_resize_area_tables(R_, C_, H, W, ptr(xf), ptr(xc), ptr(xw), ptr(yf), ptr(yc), ptr(yw), C.byref(whole), C.byref(scale)) == 0
    wofs = lambda c: (np.cumsum(c) - c).astype(np.int32)
    dev = [torch.from_numpy(a).cuda() for a in (xf, xc, wofs(xc), xw, yf, yc, wofs(yc), yw)]
    p = AreaParams(frames.data_ptr(), C_ * 3, R_ * C_ * 3, dst.data_ptr(), W * 3, H * W * 3, R_, C_, H, W, 3, N, whole.value, scale.value,
                   *[d.data_ptr() for d in dev])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        assert launch(C.byref(p), stream, None)
    return run, "area_reduce_kernel<3, %s>" % ("true" if whole.value else "false"), (dev, p)


def aa_launch(lib, name, frames, dst):
    launch = getattr(C.CDLL(B.kernel_library("aa").out), "_ZN3rip9launch_aaERKNS_8AaParamsERKNS_9FitWindowEP12ihipStream_tPNS_10LaunchInfoE")
    launch.restype = C.c_bool
    S = 2 if name == "cubic_aa" else 1
    xf, xc, xo, xw = np.zeros(W, np.int32), np.zeros(W, np.int32), np.zeros(W, np.int32), np.zeros(2 * S * C_ + W, np.int16)
    yf, yc, yo, yw = np.zeros(H, np.int32), np.zeros(H, np.int32), np.zeros(H, np.int32), np.zeros(2 * S * R_ + H, np.int16)
    xprec, yprec, th, rows = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    assert lib.rip_debug_resize_aa_tables(name.encode(), R_, C_, H, W, 3, ptr(xf), ptr(xc), ptr(xo), ptr(xw), ptr(yf), ptr(yc), ptr(yo), ptr(yw),
                                          C.byref(xprec), C.byref(yprec), C.byref(th), C.byref(rows)) == 0
    dev = [torch.from_numpy(a).cuda() for a in (xf, xc, xo, xw, yf, yc, yo, yw)]
    p = AaParams(frames.data_ptr(), C_ * 3, R_ * C_ * 3, dst.data_ptr(), W * 3, H * W * 3, R_, C_, H, W, 3, N, th.value, rows.value, xprec.value, yprec.value,
                 *[d.data_ptr() for d in dev])
    w = FitWindow(0, 0, C_, R_)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        assert launch(C.byref(p), C.byref(w), stream, None)
    return run, "aa_kernel<3, false> TH=%d, %d LDS rows (%d bytes)" % (th.value, rows.value, rows.value * 64 * 3), (dev, p, w)


def main():
    import aa_reference as A
    import area_reference as AR
    lib = load_library()
    g = torch.Generator(device="cuda").manual_seed(1)
    frames = torch.randint(0, 256, (N, R_, C_, 3), dtype=torch.uint8, device="cuda", generator=g)
    say("frames %d x %d x %d x 3 uint8 = %.1f MB resident -> %d x %d; HIP events around 4 launches, 5 rounds per leg, the legs alternating, after 2 "
        "warm-up launches each; ms per launch of %d frames" % (N, R_, C_, frames.numel() / 1e6, W, H, N))
    dsts = [torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(3)]
    legs = [("linear_aa",) + aa_launch(lib, "linear_aa", frames, dsts[0]), ("cubic_aa",) + aa_launch(lib, "cubic_aa", frames, dsts[1]),
            ("area",) + area_launch(lib, frames, dsts[2])]
    for _, run, _, _ in legs:
        run()
        run()
    torch.cuda.synchronize()
    f3 = frames[3].cpu().numpy()
    assert np.array_equal(dsts[0][3].cpu().numpy(), A.resize(f3, H, W, "linear_aa")), "timed linear_aa kernel differs from the reference"
    assert np.array_equal(dsts[1][3].cpu().numpy(), A.resize(f3, H, W, "cubic_aa")), "timed cubic_aa kernel differs from the reference"
    assert np.array_equal(dsts[2][3].cpu().numpy(), AR.resize(f3, H, W)), "timed area kernel differs from the reference"
    times = {name: [] for name, _, _, _ in legs}
    for _ in range(5):
        for name, run, _, _ in legs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(4):
                run()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / 4)
    nbytes = N * 3 * (R_ * C_ + H * W)
    say("%-10s %-58s %9s %9s %9s  %s" % ("filter", "kernel", "median", "min", "max", "GB/s on 3RC + 3HW bytes per frame (median)"))
    for name, _, kernel, _ in legs:
        t = times[name]
        med = float(np.median(t))
        say("%-10s %-58s %9.3f %9.3f %9.3f  %.0f" % (name, kernel, med, min(t), max(t), nbytes / med / 1e6))
    say("done")


if __name__ == "__main__":
    main()
