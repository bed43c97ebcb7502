"""Map build time on the device for a pinhole calibration (plumb_bob: rip_maps.hip pinhole_maps_kernel) next to the fisheye
builder's at the same size: wall time of init_undistortion() after a balance change dirtied the maps (map kernels, stream
synchronisation; the remap plan is compiled by the first frame, not here), median and minimum of 20 after 3 warm-up calls, and
the same with RIP_MAPS_ON_HOST=1 (the host builders on up to 16 threads plus the upload)."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
from raw_image_pipeline_amd import RawImagePipeline, synth  # noqa: E402

W, H = 2448, 2048
CAMERAS = (("equidistant", synth.camera_model(W, H)),
           ("plumb_bob", synth.pinhole_camera_model(W, H, [-0.28, 0.07, 2e-4, -3e-4, 0.0])),
           ("rational_polynomial", synth.pinhole_camera_model(W, H, [0.9, 0.25, 3e-4, -2e-4, 0.01, 1.25, 0.55, 0.05])))
for mode in ("device", "host"):
    if mode == "host":
        os.environ["RIP_MAPS_ON_HOST"] = "1"
    else:
        os.environ.pop("RIP_MAPS_ON_HOST", None)
    for model, cam in CAMERAS:
        p = RawImagePipeline(False, "", "", "", device=0)
        synth.load_camera(p, cam, model)
        p.set_undistortion(True)
        ts = []
        for rep in range(23):
            p.set_undistortion_balance(0.04 * rep)  # dirties the maps
            torch.cuda.synchronize()
            t = time.perf_counter()
            p.init_undistortion()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        ts = ts[3:]
        print("%dx%d %-6s %-20s init_undistortion: median %.3f ms, min %.3f ms (n = %d)" % (W, H, mode, model, statistics.median(ts), min(ts), len(ts)))
