"""The order in which the ring remap kernels visit the tiles of a run (Tunables::remap_order, csrc/rip_tile_deal.hpp) decides which
workgroup takes a tile and when, never what it computes: every order x run length gives the bytes of the row-major walk, and
those are the oracle's (tolerance 0).  Two paths, because each sends the tiles through another kernel: chain + fisheye remap
(remap_ring_kernel behind an intermediate image) and debayer + remap in one kernel (remap_bayer_ring_kernel).

Shapes that make the mapping ragged (tiles are 64 x 16):
  64 x 16     one tile
  200 x 72    a partial last tile column and 4.5 tile rows: the last run is shorter than the strip
  328 x 144   9 tile rows: one full run of 8 plus a ragged one, and fewer than 8 runs, so XCDs without work
  1000 x 752  16 x 47 tiles, enough of them that a visit holds several frames: five frames in visits of 3 + 2 (4 frames per
              visit asked for) and 2 + 2 + 1 (2 asked for); the smaller plans split a batch of five into one-frame visits
Batches of five frames throughout: batches below four frames take the contiguous deal, which has no runs to order."""
import numpy as np
import pytest

from helpers import GENERIC_KERNELS, assert_images_equal, assert_launched, cfg, configure, device_batch, oracle_run
from raw_image_pipeline_amd import synth

pytestmark = pytest.mark.gpu

N_FRAMES = 5
SIZES = [(64, 16), (200, 72), (328, 144), (1000, 752)]
RUNS = (1, 2, 3, 4, 8, 16)          # remap_deal, tile rows per run; 3: column strips round it down to 2
FRAMES_PER_VISIT = (0, 2, 4)        # remap_frames; 0: the launcher's rule
_ORACLE = {}


def oracle_frames(O, c, frames, encoding, key, which):
    """The oracle's images of frames[which], computed once per (path, size)."""
    if key not in _ORACLE:
        _ORACLE[key] = {i: oracle_run(O, c, frames[i], encoding)[0] for i in which}
    return _ORACLE[key]


def sweep_orders(pipe, O, c, frames, dev, what, launched, key):
    import torch
    configure(pipe, c)
    shape = tuple(pipe.apply_device(dev, "bayer_rggb8").shape)

    def run():
        out = torch.full(shape, 0x5A, dtype=torch.uint8, device="cuda")  # a tile no workgroup took must not pass on recycled bytes
        pipe.apply_device(dev, "bayer_rggb8", out=out)
        return out.cpu().numpy()

    pipe.set_tunable("remap_order", 0)
    base = run()
    w, h = frames.shape[2], frames.shape[1]
    which = range(N_FRAMES) if w * h <= 328 * 144 else (0, N_FRAMES - 1)
    for i, ref in oracle_frames(O, c, frames, "bayer_rggb8", key, which).items():
        assert_images_equal(base[i].reshape(ref.shape), ref, "row-major, default run vs oracle, %s frame %d" % (what, i), 0)
    for frames_per_visit in FRAMES_PER_VISIT:
        pipe.set_tunable("remap_frames", frames_per_visit)
        for run_rows in RUNS:
            pipe.set_tunable("remap_deal", run_rows)
            for order in (0, 1, 2):   # 2: column strips where they deal out evenly over the XCDs, row-major elsewhere
                pipe.set_tunable("remap_order", order)
                with pipe.launch_log() as log:
                    got = run()
                assert np.array_equal(got, base), "%s: remap_order %d remap_deal %d remap_frames %d changes the image" % (what, order, run_rows, frames_per_visit)
                assert_launched(log, launched, GENERIC_KERNELS, "%s order %d run %d" % (what, order, run_rows))


def make_frames(w, h):
    return np.stack([synth.gen_frame(w, h, "bayer_rggb8", seed=4100 + i, kind="scene") for i in range(N_FRAMES)])


@pytest.mark.parametrize("size", SIZES)
def test_chain_and_ring_remap_give_the_same_bytes_under_every_order_and_run_length(gpu_pipe, oracle, size):
    """The full chain (statistics, fused chain with vignetting, intermediate image) and the fisheye ring remap behind it."""
    import torch
    w, h = size
    c = cfg(flip=True, flip_angle=180, wb=True, wb_method="grey_world", cc=True, gamma=True, gamma_k=0.8, vig=True, undistort=True,
            cam=synth.camera_model(w, h))
    frames = make_frames(w, h)
    dev = torch.from_numpy(frames).cuda()
    sweep_orders(gpu_pipe, oracle, c, frames, dev, "two kernels %dx%d" % size, ["chain_fast_kernel<*>", "remap_ring_kernel<?, 3, false>"], ("two", size))


@pytest.mark.parametrize("size", SIZES)
def test_the_fused_debayer_and_remap_gives_the_same_bytes_under_every_order_and_run_length(gpu_pipe, oracle, size):
    """Debayer + gains + matrix + gamma + undistortion without a tap: the remap's tiles demosaic and colour their own source
    rectangles (remap_bayer_ring_kernel).  That kernel asks for a Bayer row pitch that is a multiple of 16, so the frames are
    handed over as a pitched view (helpers.device_batch "pitch16") and no chain kernel may run."""
    w, h = size
    c = cfg(flip=True, flip_angle=180, wb=True, wb_method="grey_world", cc=True, gamma=True, gamma_k=0.8, undistort=True, cam=synth.camera_model(w, h))
    frames = make_frames(w, h)
    batch = device_batch(frames, "pitch16", np.random.default_rng(w))
    assert batch.pitch % 16 == 0
    sweep_orders(gpu_pipe, oracle, c, frames, batch.view, "fused %dx%d" % size, ["remap_bayer_ring_kernel<*>"], ("fused", size))
    batch.check_padding("fused %dx%d" % size)
