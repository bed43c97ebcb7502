#!/usr/bin/env python3
"""Probe: cost of the resize launch (rip_set_output_size, csrc/rip_resize.hip) on the MI355X: 256 resident 2448 x 2048 bgr8 results
-> 640 x 512, -> 1224 x 1024 (the 2 x 2 mean), -> rgb_chw_f16 at 640 x 512, against what a consumer does today: native delivery +
torch.nn.functional.interpolate(mode="bilinear") (not bit-identical).  HIP events, warm-up excluded, median / min.

Legs, all in one process on the same seeded frames: the kernel alone (rip::launch_resize of librip_rsz_hip.so called directly on
host-built tables; one frame of each shape is compared with the oracle first), rip_apply_device with and without a target and a
format, and the torch expressions.  Every line printed is also written to the output file.
Usage: resize_probe.py [OUT.txt]   (default profiles/resize_kernel_times.txt)

resize_probe.py --interpolation [OUT.txt] (default profiles/resize_area_kernel_times.txt) is another run: the launches alone of the
area interpolation (rip::launch_area_reduce of librip_area_hip.so; at exactly half size the 2 x 2 mean kernel of librip_rsz_hip.so)
and of the linear kernel at the same three targets -- 612 x 512 (whole 4 x 4), 640 x 480 (tap lists), 1224 x 1024 (2 x 2) -- on the
same resident batch, alternating the two filters; each time with its spread and the fraction of 8 TB/s it stands for on
3 R C + 3 H W bytes per frame.  One frame of every area launch is compared with tests/area_reference.py first.

resize_probe.py --fit [OUT.txt] (default profiles/resize_fit_times.txt) is a third run: rip_apply_device on the same resident batch
with every stage off, 2448 x 2048 -> 640 x 480 under "stretch", "letterbox" and "crop" (rip_set_output_fit), linear and area, the
six settings alternating on one handle; one frame of each is compared with tests/fit_reference.py first.  The stretch legs read
all of the image through the existing kernels; crop reads a window through librip_fit_hip.so; letterbox adds the pad launch."""
import ctypes as C
import os
import sys
import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from raw_image_pipeline_amd import RawImagePipeline, load_library  # noqa: E402
from raw_image_pipeline_amd import build as B  # noqa: E402

N, R_, C_ = 256, 2048, 2448
INTERPOLATION = "--interpolation" in sys.argv[1:]
FIT = "--fit" in sys.argv[1:]
ARGS = [a for a in sys.argv[1:] if a not in ("--interpolation", "--fit")]
OUT = open(ARGS[0] if ARGS else os.path.join(ROOT, "profiles", "resize_fit_times.txt" if FIT else
                                             "resize_area_kernel_times.txt" if INTERPOLATION else "resize_kernel_times.txt"), "w")


def say(line):
    print(line, flush=True)
    OUT.write(line + "\n")
    OUT.flush()


def timed(fn, warm=2, reps=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


class ResizeParams(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_step", C.c_size_t), ("src_frame_stride", C.c_size_t), ("dst", C.c_void_p), ("dst_step", C.c_size_t),
                ("dst_frame_stride", C.c_size_t), ("src_rows", C.c_int), ("src_cols", C.c_int), ("rows", C.c_int), ("cols", C.c_int),
                ("channels", C.c_int), ("n_frames", C.c_int), ("area2", C.c_int), ("xofs", C.c_void_p), ("alpha", C.c_void_p), ("yofs", C.c_void_p),
                ("beta", C.c_void_p)]


class AreaParams(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_step", C.c_size_t), ("src_frame_stride", C.c_size_t), ("dst", C.c_void_p), ("dst_step", C.c_size_t),
                ("dst_frame_stride", C.c_size_t), ("src_rows", C.c_int), ("src_cols", C.c_int), ("rows", C.c_int), ("cols", C.c_int),
                ("channels", C.c_int), ("n_frames", C.c_int), ("whole", C.c_int), ("scale", C.c_float), ("xfirst", C.c_void_p), ("xcount", C.c_void_p),
                ("xwofs", C.c_void_p), ("xweight", C.c_void_p), ("yfirst", C.c_void_p), ("ycount", C.c_void_p), ("ywofs", C.c_void_p), ("yweight", C.c_void_p)]


def linear_launch(lib, rsz, frames, dst, H, W):
    """(callable that enqueues resize_kernel on the current stream, kernel name, objects to keep alive)"""
    launch = getattr(rsz, "_ZN3rip13launch_resizeERKNS_12ResizeParamsEP12ihipStream_tPNS_10LaunchInfoE")
    launch.restype = C.c_bool
    wp = (W + 3) // 4 * 4
    xofs, alpha = np.zeros(wp, np.int32), np.zeros((wp, 2), np.int16)
    yofs, beta = np.zeros((H, 2), np.int32), np.zeros((H, 2), np.int16)
    area = C.c_int(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.rip_debug_resize_tables(R_, C_, H, W, ptr(xofs), ptr(alpha), ptr(yofs), ptr(beta), C.byref(area)) == 0
    dev = [torch.from_numpy(a).cuda() for a in (xofs, alpha, yofs, beta)]
    p = ResizeParams(frames.data_ptr(), C_ * 3, R_ * C_ * 3, dst.data_ptr(), W * 3, H * W * 3, R_, C_, H, W, 3, N, area.value,
                     dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        assert launch(C.byref(p), stream, None)
    return run, "resize_kernel<3, %s>" % ("true" if area.value else "false"), (dev, p)


def area_launch(lib, frames, dst, H, W):
    launch = getattr(C.CDLL(B.kernel_library("area").out), "_ZN3rip18launch_area_reduceERKNS_10AreaParamsEP12ihipStream_tPNS_10LaunchInfoE")
    launch.restype = C.c_bool
    xf, xc, xw = np.zeros(W, np.int32), np.zeros(W, np.int32), np.zeros(C_ + 2 * W, np.float32)
    yf, yc, yw = np.zeros(H, np.int32), np.zeros(H, np.int32), np.zeros(R_ + 2 * H, np.float32)
    whole, scale = C.c_int(0), C.c_float(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.rip_debug_resize_area_tables(R_, C_, H, W, ptr(xf), ptr(xc), ptr(xw), ptr(yf), ptr(yc), ptr(yw), C.byref(whole), C.byref(scale)) == 0
    wofs = lambda c: (np.cumsum(c) - c).astype(np.int32)
    dev = [torch.from_numpy(a).cuda() for a in (xf, xc, wofs(xc), xw, yf, yc, wofs(yc), yw)]
    p = AreaParams(frames.data_ptr(), C_ * 3, R_ * C_ * 3, dst.data_ptr(), W * 3, H * W * 3, R_, C_, H, W, 3, N, whole.value, scale.value,
                   *[d.data_ptr() for d in dev])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        assert launch(C.byref(p), stream, None)
    return run, "area_reduce_kernel<3, %s>" % ("true" if whole.value else "false"), (dev, p)


def interpolation_main():
    """The three-target table, area against linear: launches alone, the two filters alternating, 5 rounds of 4 launches each after a
    warm-up of 2 launches per kernel."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import area_reference as A
    lib = load_library()
    rsz = C.CDLL(B.kernel_library("rsz").out)
    g = torch.Generator(device="cuda").manual_seed(1)
    frames = torch.randint(0, 256, (N, R_, C_, 3), dtype=torch.uint8, device="cuda", generator=g)
    say("frames %d x %d x %d x 3 uint8 = %.1f MB resident; HIP events around 4 launches, 5 rounds per kernel alternating area / linear, after 2 "
        "warm-up launches each; ms per launch of %d frames" % (N, R_, C_, frames.numel() / 1e6, N))
    say("%-12s %-8s %-30s %9s %9s %9s  %s" % ("target", "filter", "kernel", "median", "min", "max", "share of 8 TB/s on 3RC + 3HW bytes per frame (median)"))
    for (W, H, path) in ((612, 512, "whole 4 x 4"), (640, 480, "tap lists"), (1224, 1024, "2 x 2 mean")):
        dsts = [torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
        legs = []
        if (R_, C_) == (2 * H, 2 * W):
            legs.append(("area",) + linear_launch(lib, rsz, frames, dsts[0], H, W))      # the area setting routes this size to the mean kernel
        else:
            legs.append(("area",) + area_launch(lib, frames, dsts[0], H, W))
        legs.append(("linear",) + linear_launch(lib, rsz, frames, dsts[1], H, W))
        for _, run, _, _ in legs:
            run()
            run()
        torch.cuda.synchronize()
        assert np.array_equal(dsts[0][3].cpu().numpy(), A.resize(frames[3].cpu().numpy(), H, W)), "timed area kernel differs from the reference"
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
        for name, _, kernel, _ in legs:
            t = times[name]
            med = float(np.median(t))
            say("%-12s %-8s %-30s %9.3f %9.3f %9.3f  %.3f (%s; %.0f GB/s)" % ("%dx%d" % (W, H), name, kernel, med, min(t), max(t),
                                                                              nbytes / (med * 1e-3) / 8e12, path, nbytes / med / 1e6))
        del dsts, legs
    say("done")


def fit_main():
    """2448 x 2048 -> 640 x 480 through rip_apply_device under the three fit modes and both filters, 5 rounds of 2 calls each per
    setting, the settings alternating, after a warm-up call each."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fit_reference as FR
    W, H = 640, 480
    g = torch.Generator(device="cuda").manual_seed(1)
    frames = torch.randint(0, 256, (N, R_, C_, 3), dtype=torch.uint8, device="cuda", generator=g)
    pipe = RawImagePipeline(False, "", "", "", device=0)
    for s in ("set_white_balance", "set_undistortion", "set_vignetting_correction", "set_color_calibration", "set_gamma_correction", "set_color_enhancer",
              "set_flip"):
        getattr(pipe, s)(False)
    pipe.set_output_size(W, H)
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
    say("frames %d x %d x %d x 3 uint8 = %.1f MB resident, every stage off; rip_apply_device -> %d x %d; HIP events around 2 calls, 5 rounds per "
        "setting, the six settings alternating, after a warm-up call each; ms per call of %d frames" % (N, R_, C_, frames.numel() / 1e6, W, H, N))
    legs = [(fit, interp) for interp in ("linear", "area") for fit in ("stretch", "letterbox", "crop")]

    def call(fit, interp):
        pipe.set_output_fit(fit)
        pipe.set_output_interpolation(interp)
        pipe.apply_device(frames, "bgr8", out=out)
    host = frames[3].cpu().numpy()
    kernels = {}
    for fit, interp in legs:
        with pipe.launch_log() as log:
            call(fit, interp)
            torch.cuda.synchronize()
        kernels[fit, interp] = " + ".join(n for n in log.names() if n.startswith(("fit_", "resize_kernel", "area_reduce_kernel")))
        assert np.array_equal(out[3].cpu().numpy(), FR.expected(host, None, (W, H), fit, interp)), "the timed call differs from the reference: %s %s" % (fit, interp)
    times = {leg: [] for leg in legs}
    for _ in range(5):
        for leg in legs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call(*leg)
            call(*leg)
            b.record()
            b.synchronize()
            times[leg].append(a.elapsed_time(b) / 2)
    say("%-10s %-8s %9s %9s %9s %9s  %s" % ("fit", "filter", "median", "min", "max", "/stretch", "window read, picture written, kernels of the stage"))
    for fit, interp in legs:
        t, base = times[fit, interp], float(np.median(times["stretch", interp]))
        src, dst = pipe.set_output_fit(fit) or pipe.get_output_window(R_, C_, 3, "bgr8")
        say("%-10s %-8s %9.3f %9.3f %9.3f %9.3f  %s -> %s, %s" % (fit, interp, float(np.median(t)), min(t), max(t), float(np.median(t)) / base, src, dst,
                                                               kernels[fit, interp]))
    say("done")


def main():
    if FIT:
        return fit_main()
    if INTERPOLATION:
        return interpolation_main()
    lib = load_library()
    rsz = C.CDLL(B.kernel_library("rsz").out)
    launch = getattr(rsz, "_ZN3rip13launch_resizeERKNS_12ResizeParamsEP12ihipStream_tPNS_10LaunchInfoE")
    launch.restype = C.c_bool
    g = torch.Generator(device="cuda").manual_seed(1)
    frames = torch.randint(0, 256, (N, R_, C_, 3), dtype=torch.uint8, device="cuda", generator=g)
    say("frames %d x %d x %d x 3 uint8 = %.1f MB; HIP events, median / min of 7 after 2 warm-up runs" % (N, R_, C_, frames.numel() / 1e6))

    # ---- the kernel alone ----
    for (W, H) in ((640, 512), (1224, 1024)):
        wp = (W + 3) // 4 * 4
        xofs, alpha = np.zeros(wp, np.int32), np.zeros((wp, 2), np.int16)
        yofs, beta = np.zeros((H, 2), np.int32), np.zeros((H, 2), np.int16)
        area = C.c_int(0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.rip_debug_resize_tables(R_, C_, H, W, ptr(xofs), ptr(alpha), ptr(yofs), ptr(beta), C.byref(area)) == 0
        dev = [torch.from_numpy(a).cuda() for a in (xofs, alpha, yofs, beta)]
        dst = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
        p = ResizeParams(frames.data_ptr(), C_ * 3, R_ * C_ * 3, dst.data_ptr(), W * 3, H * W * 3, R_, C_, H, W, 3, N, area.value,
                         dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def run():
            assert launch(C.byref(p), stream, None)
        med, best = timed(run)
        read_min = N * H * W * 3 * 4 if not area.value else N * R_ * C_ * 3
        written = N * H * W * 3
        say("resize_kernel<3, %s> %dx%d -> %dx%d, %d frames: median %.3f ms, min %.3f ms; written %.1f MB, taps read %.1f MB, source image %.1f MB; "
            "(taps + written) / min = %.0f GB/s" % ("true" if area.value else "false", C_, R_, W, H, N, med, best, written / 1e6, read_min / 1e6,
                                                     N * R_ * C_ * 3 / 1e6, (read_min + written) / best / 1e6))
        # one frame against the CPU definition, so that the timed kernel is the right one
        import oracle as O
        O.build()
        ref = O.resize_linear(frames[3].cpu().numpy(), H, W)
        assert np.array_equal(dst[3].cpu().numpy(), ref), "timed kernel differs from the oracle"

    # ---- through the library: apply_device on resident bgr8 frames with every stage off ----
    pipe = RawImagePipeline(False, "", "", "", device=0)
    for s in ("set_white_balance", "set_undistortion", "set_vignetting_correction", "set_color_calibration", "set_gamma_correction", "set_color_enhancer",
              "set_flip"):
        getattr(pipe, s)(False)
    results = {}
    for name, fmt, target in (("native, no target", "native", (0, 0)), ("native -> 640x512", "native", (640, 512)), ("native -> 1224x1024", "native", (1224, 1024)),
                              ("rgb_chw_f16, no target", "rgb_chw_f16", (0, 0)), ("rgb_chw_f16 -> 640x512", "rgb_chw_f16", (640, 512))):
        pipe.set_output_format(fmt)
        pipe.set_output_size(*target)
        out = pipe.apply_device(frames, "bgr8")
        med, best = timed(lambda: pipe.apply_device(frames, "bgr8", out=out))
        results[name] = (med, best)
        say("apply_device %-26s median %.3f ms, min %.3f ms (%s %s)" % (name + ":", med, best, tuple(out.shape), out.dtype))
        del out
    pipe.set_output_size(0, 0)
    pipe.set_output_format("native")
    native = pipe.apply_device(frames, "bgr8")
    torch.cuda.synchronize()

    # ---- what a consumer does today: native delivery, then torch's bilinear interpolation (not bit-identical) ----
    def torch_resize(size, half):
        x = native.permute(0, 3, 1, 2).float()
        y = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
        if half:
            y = (y.flip(1) / 255.0).half()
        return y
    for name, size, half in (("uint8 NHWC -> float NCHW -> bilinear 640x512", (512, 640), False), ("... -> bilinear 1224x1024", (1024, 1224), False),
                             ("... -> bilinear 640x512 -> rgb / 255 -> f16", (512, 640), True)):
        med, best = timed(lambda: torch_resize(size, half), warm=2, reps=5)
        say("torch %-50s median %.3f ms, min %.3f ms" % (name + ":", med, best))
    x = native.permute(0, 3, 1, 2).float()
    med, best = timed(lambda: F.interpolate(x, size=(512, 640), mode="bilinear", align_corners=False), warm=2, reps=5)
    say("torch %-50s median %.3f ms, min %.3f ms" % ("interpolate alone on a float NCHW tensor, 640x512:", med, best))
    med, best = timed(lambda: F.interpolate(x, size=(1024, 1224), mode="bilinear", align_corners=False), warm=2, reps=5)
    say("torch %-50s median %.3f ms, min %.3f ms" % ("interpolate alone on a float NCHW tensor, 1224x1024:", med, best))
    say("done")


if __name__ == "__main__":
    main()
