"""Seeded random configurations where the first fuzz (tests/test_fuzz_gpu.py) does not go, HIP against the CPU at tolerance 0:

1. the "mht" debayer method under any configuration, at sizes around the edges of its 64 x 32 tiles, single frames with both taps
   and resident batches of up to 17 frames (several frame groups of the tile kernel), with and without a debayered tap (without
   one the MHT image lies in the handle's buffer with padded rows and feeds the colour kernels as a pitched bgr8 image);
2. the bilinear path and colour / mono input in batches that cross the frames-per-visit boundaries of every kernel (up to 33
   frames);
3. the footprint walk of the fused chain in front of the remap with an off-centre camera, asserting which walk ran.

Every batch is a strided view in one of five layouts (helpers.device_batch): tightly packed, padded rows (16-byte aligned and
not aligned at all), a base address off the dword grid, spare rows between frames; the bytes around the frames hold a sentinel
and must still hold it afterwards.  The expectation of an MHT frame is the oracle on the numpy restatement of the demosaic
(helpers.expected_mht) -- no second GPU handle is involved.  tests/test_fuzz_layout_cases.py checks the generators on the CPU."""
import numpy as np
import pytest

import fuzz_layout_cases as G
from helpers import assert_images_equal, configure, device_batch, expected_mht, oracle_run
from raw_image_pipeline_amd import synth

pytestmark = pytest.mark.gpu


def tap_shape(case):
    w, h = case["w"], case["h"]
    ow, oh = (h, w) if case["flip"] in (90, 270) else (w, h)
    return (case["n"], oh, ow, 3)


@pytest.mark.parametrize("seed", range(G.N_MHT))
def test_random_mht_configuration(gpu_pipe, oracle, seed):
    import torch
    case = G.mht_case(seed)
    w, h, pattern, c, n = case["w"], case["h"], case["pattern"], case["c"], case["n"]
    what = "mht " + G.describe(case)
    configure(gpu_pipe, c)
    gpu_pipe.set_debayer_method("mht")
    # (a) one host frame, both taps
    frame = synth.gen_frame(w, h, pattern, seed=seed, kind=case["kind"], tint=case["tint"])
    got = gpu_pipe.process(frame, pattern)
    assert gpu_pipe.last_encoding == "bgr8"
    ref, enc, t_deb, t_col = expected_mht(oracle, c, frame, pattern, taps=True)
    assert enc == "bgr8"
    assert_images_equal(got, ref, what)
    assert_images_equal(gpu_pipe.get_dist_debayered_image(), t_deb.reshape(gpu_pipe.get_dist_debayered_image().shape), what + " debayered tap")
    assert_images_equal(gpu_pipe.get_dist_color_image(), t_col.reshape(gpu_pipe.get_dist_color_image().shape), what + " colour tap")
    # (b) a resident batch in the case's layout, frames all different
    frames = np.stack([synth.gen_frame(w, h, pattern, seed=1000 * seed + 7 + i, kind=case["kind"] if i % 3 else "uniform") for i in range(n)])
    assert len({f.tobytes() for f in frames}) == n
    batch = device_batch(frames, case["layout"], np.random.default_rng(case["layout_seed"]))
    tap = torch.full(tap_shape(case), 0x5A, dtype=torch.uint8, device="cuda") if case["tap"] else None
    out = gpu_pipe.apply_device(batch.view, pattern, tap_debayered=tap)
    batch.check_padding(what)
    out = out.cpu().numpy()
    tap = tap.cpu().numpy() if tap is not None else None
    for i in range(n):
        ref, _, t_deb, _ = expected_mht(oracle, c, frames[i], pattern, taps=True)
        assert_images_equal(out[i], ref, what + " batch frame %d/%d" % (i, n))
        if tap is not None:
            assert_images_equal(tap[i], t_deb.reshape(tap[i].shape), what + " debayered tap of batch frame %d/%d" % (i, n))


@pytest.mark.parametrize("seed", range(G.N_LAYOUT))
def test_random_layout_configuration(gpu_pipe, oracle, seed):
    case = G.layout_case(seed)
    w, h, encoding, c, n = case["w"], case["h"], case["encoding"], case["c"], case["n"]
    what = G.describe(case)
    rng = np.random.default_rng(case["layout_seed"])
    if encoding.startswith("bayer"):
        frames = [synth.gen_frame(w, h, encoding, seed=1000 * seed + i, kind=case["kind"] if i % 3 else "uniform") for i in range(n)]
    elif encoding == "mono8":
        frames = [rng.integers(0, 256, (h, w), dtype=np.uint8) for i in range(n)]
    else:
        frames = [synth.gen_scene_bgr(w, h, seed=1000 * seed + i) if i % 2 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for i in range(n)]
    frames = np.stack(frames)
    assert len({f.tobytes() for f in frames}) == n
    configure(gpu_pipe, c)
    batch = device_batch(frames, case["layout"], rng)
    out = gpu_pipe.apply_device(batch.view, encoding)
    batch.check_padding(what)
    out = out.cpu().numpy()
    for i in range(n):
        ref, _ = oracle_run(oracle, c, frames[i], encoding)
        assert_images_equal(out[i].reshape(ref.shape), ref, what + " batch frame %d/%d" % (i, n))


@pytest.mark.parametrize("seed", range(G.N_FOOTPRINT))
def test_random_footprint_walk(gpu_pipe, oracle, seed):
    import torch
    case = G.footprint_case(seed)
    w, h, pattern, c, n = case["w"], case["h"], case["pattern"], case["c"], case["n"]
    what = "footprint " + G.describe(case)
    angle = c["flip_angle"] if c["flip"] else 0
    frames = np.stack([synth.gen_frame(w, h, pattern, seed=1000 * seed + i, kind=case["kind"] if i % 3 else "uniform") for i in range(n)])
    configure(gpu_pipe, c)
    batch = device_batch(frames, case["layout"], np.random.default_rng(case["layout_seed"]))
    gpu_pipe.set_tunable("chain_footprint", 1)
    got = gpu_pipe.apply_device(batch.view, pattern)
    batch.check_padding(what)
    info, _ = gpu_pipe.debug_chain_footprint(h, w, angle)
    assert info["dense_items"] == (h // 2) * (w // 4)
    # which walk ran, not only what it produced: the item list up to 95 % of the frame, the dense walk above
    listed = info["footprint_items"] <= 0.95 * info["dense_items"]
    assert info["last_walked"] == (info["footprint_items"] if listed else info["dense_items"]), (what, info)
    gpu_pipe.set_tunable("chain_footprint", 0)
    dense = gpu_pipe.apply_device(batch.view, pattern)
    batch.check_padding(what + " dense")
    assert gpu_pipe.debug_chain_footprint(h, w, angle)[0]["last_walked"] == info["dense_items"]
    assert torch.equal(got, dense), "%s: footprint walk differs from the dense walk on %d bytes" % (what, int((got != dense).sum()))
    got = got.cpu().numpy()
    for i in range(n):
        ref, _ = oracle_run(oracle, c, frames[i], pattern)
        assert_images_equal(got[i], ref, what + " batch frame %d/%d" % (i, n))
