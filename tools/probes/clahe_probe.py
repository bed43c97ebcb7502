"""The two CLAHE kernels (csrc/rip_clahe.hip) at 2448 x 2048, one channel, tiles (8, 8), clip limit 3: 256 resident frames and one
frame, on scenes and on flat frames.  Run under the profiler, then summarise its kernel trace with the warm-up calls left out:

    rocprofv3 --kernel-trace --stats -d out -o clahe -- python tools/probes/clahe_probe.py run
    python tools/probes/clahe_probe.py summarise out/.../clahe_kernel_trace.csv

A handle with every stage off delivers the mono frames as they are, so the two kernels are all that follows the chain's copy.  The 256
scene frames are 8 generated scenes repeated 32 times: the kernels see 256 different addresses, the contents repeat."""
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

W, H, TILES, CLIP = 2448, 2048, (8, 8), 3.0
# (frames, content, warm-up calls, timed calls), in the order they run
CONFIGS = [(256, "scene", 2, 5), (256, "flat", 2, 5), (1, "scene", 3, 20), (1, "flat", 3, 20)]
KERNELS = ("clahe_lut_kernel", "clahe_apply_kernel")


def run():
    import numpy as np
    import torch
    from raw_image_pipeline_amd import RawImagePipeline, synth
    p = RawImagePipeline(False, "", "", "", device=0)
    for off in (p.set_flip, p.set_white_balance, p.set_color_calibration, p.set_gamma_correction, p.set_vignetting_correction, p.set_color_enhancer,
                p.set_undistortion):
        off(False)
    p.set_output_clahe(CLIP, *TILES)
    scenes = np.stack([synth.gen_scene_bgr(W, H, seed)[..., 1] for seed in range(8)])
    for n, content, warm, timed in CONFIGS:
        if content == "flat":
            frames = torch.full((n, H, W), 100, dtype=torch.uint8, device="cuda")
        else:
            frames = torch.from_numpy(scenes[:min(n, 8)]).cuda().repeat((n + 7) // 8, 1, 1)[:n].contiguous()
        out = torch.empty_like(frames)
        for _ in range(warm + timed):
            p.apply_device(frames, "mono8", out=out)
        torch.cuda.synchronize()
        print("%d frames %s: done, mean of the result %.2f" % (n, content, float(out[0].float().mean())))


def summarise(path):
    rows = {k: [] for k in KERNELS}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    rows[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    px = W * H
    print("CLAHE kernels at %d x %d, tiles %r, clip limit %g; microseconds per launch, warm-up calls excluded" % (W, H, TILES, CLIP))
    print("%-20s %6s %-6s %5s %10s %10s %10s %12s %10s" % ("kernel", "frames", "what", "calls", "average", "min", "max", "bytes moved", "bytes/s"))
    for k in KERNELS:
        calls = [e - s for s, e in sorted(rows[k])]
        assert len(calls) == sum(w + t for _, _, w, t in CONFIGS), (k, len(calls))
        at = 0
        for n, content, warm, timed in CONFIGS:
            us = [c / 1e3 for c in calls[at + warm:at + warm + timed]]
            at += warm + timed
            moved = n * px * (1 if k == KERNELS[0] else 2) + n * TILES[0] * TILES[1] * 256
            avg = sum(us) / len(us)
            print("%-20s %6d %-6s %5d %10.1f %10.1f %10.1f %9.1f MB %7.2f TB/s" % (k, n, content, len(us), avg, min(us), max(us), moved / 1e6, moved / avg / 1e6))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "summarise":
        summarise(sys.argv[2])
    else:
        sys.exit(__doc__)
