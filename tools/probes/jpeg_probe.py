"""The four JPEG kernels (csrc/rip_jpeg.hip) at 2448 x 2048, quality 90, restart_rows 1: 256 resident frames and one frame, colour
(bgr8 scenes) and grey (their green channel), every stage of the chain off.

    python tools/probes/jpeg_probe.py run          HIP-event time of whole apply_device calls (chain copy + the four kernels), the
                                                   stream lengths, and Pillow's single-thread encode of the same pictures
    rocprofv3 --kernel-trace --stats -d DIR -o jpeg -- python tools/probes/jpeg_probe.py run
                                                   the per-kernel times (profiles/jpeg_times.txt was made from the stats file)

Needs a GPU."""
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests"))

W, H, QUALITY = 2448, 2048, 90


def main():
    import torch
    from helpers import cfg, configure
    from raw_image_pipeline_amd import RawImagePipeline, synth
    scenes = np.stack([synth.gen_scene_bgr(W, H, seed) for seed in range(4)])
    for channels in (3, 1):
        host = scenes if channels == 3 else np.ascontiguousarray(scenes[..., 1])
        enc = "bgr8" if channels == 3 else "mono8"
        p = RawImagePipeline(False, "", "", "", device=0)
        configure(p, cfg())
        p.set_output_format("jpeg")
        p.set_output_jpeg(QUALITY, 1)
        for n in (256, 1):
            frames = torch.from_numpy(host).cuda().repeat((n + 3) // 4, *([1] * (host.ndim - 1)))[:n].contiguous()
            out = None
            times = []
            for it in range(3 + 7):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = p.apply_device(frames, enc, out=out)
                e1.record()
                torch.cuda.synchronize()
                if it >= 3:
                    times.append(e0.elapsed_time(e1))
            sizes = p.jpeg_sizes()
            print("channels %d frames %3d: apply_device median %.3f ms (min %.3f) per call, %.1f us per frame; stream bytes mean %.0f min %d max %d; slot %d; overflowed %d"
                  % (channels, n, float(np.median(times)), min(times), 1e3 * float(np.median(times)) / n, sizes.mean(), sizes.min(), sizes.max(), out.shape[1], int((sizes == 0).sum())))
            del frames
        try:
            from PIL import Image
            pic = host[0][..., ::-1] if channels == 3 else host[0]
            best = 1e9
            for _ in range(3):
                buf = io.BytesIO()
                t = time.perf_counter()
                Image.fromarray(np.ascontiguousarray(pic)).save(buf, "JPEG", quality=QUALITY, subsampling=2)
                best = min(best, time.perf_counter() - t)
            print("channels %d: Pillow (libjpeg-turbo, one thread) %.2f ms per frame, %d bytes" % (channels, 1e3 * best, len(buf.getvalue())))
        except ImportError:
            print("Pillow is not installed: no CPU encode time")


if __name__ == "__main__":
    if sys.argv[1:] != ["run"]:
        sys.exit(__doc__)
    main()
