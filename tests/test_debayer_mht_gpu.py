"""The "mht" debayer method on the MI355X, at tolerance 0.

Demosaic only: against the numpy restatement of the contract (tests/mht_reference.py), flipped by the CPU oracle.  Everything
after the demosaic: an MHT frame is processed exactly like a bgr8 frame holding the MHT image, so a second handle with the same
parameters fed those bgr8 frames is the expected result -- white balance (ccc temporal state included), matrix, gamma,
vignetting, enhancer, undistortion, taps, debug dumps."""
import functools

import numpy as np
import pytest

from helpers import DUMP_NAMES, GENERIC_KERNELS, assert_images_equal, assert_launched, cfg, configure, normalize_minmax, oracle_run, read_png
from mht_reference import flip, mht_reference, phase_of
from raw_image_pipeline_amd import synth

pytestmark = pytest.mark.gpu

PATTERNS = ["bayer_rggb8", "bayer_bggr8", "bayer_gbrg8", "bayer_grbg8"]
ANGLES = [0, 90, 180, 270]


@functools.lru_cache(maxsize=32)
def frame_and_reference(w, h, pattern, seed):
    frame = synth.gen_frame(w, h, pattern, seed=seed, kind="uniform" if seed % 2 else "scene")
    return frame, mht_reference(frame, pattern)


def new_pipe(method="mht"):
    from raw_image_pipeline_amd import RawImagePipeline
    p = RawImagePipeline(False, "", "", "", device=0)
    p.set_white_balance(False)
    p.set_undistortion(False)
    p.set_debayer_method(method)
    return p


def flip_cfg(angle):
    return cfg(flip=angle != 0, flip_angle=angle)


@pytest.mark.parametrize("angle", ANGLES)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("size", [(3, 3), (7, 5), (53, 37), (645, 483), (640, 480), (2448, 2048)])
def test_demosaic_only(gpu_pipe, oracle, size, pattern, angle):
    w, h = size
    frame, mht = frame_and_reference(w, h, pattern, w % 5 + h)
    configure(gpu_pipe, flip_cfg(angle))
    gpu_pipe.set_debayer_method("mht")
    got = gpu_pipe.process(frame, pattern)
    assert gpu_pipe.last_encoding == "bgr8"
    ref, _ = oracle_run(oracle, flip_cfg(angle), mht, "bgr8")
    assert_images_equal(got, ref, "mht %s %s flip %d" % (size, pattern, angle))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("site", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_impulse_responses(gpu_pipe, pattern, site):
    ry, rx = phase_of(pattern)
    for w, h in ((14, 12), (200, 100)):  # an edge tile, and the impulse inside an interior tile of the LDS-tiled kernel
        f = np.full((h, w), 128, np.uint8)
        iy, ix = h // 2 + ((site[0] + ry) & 1), (w // 2 // 4) * 4 + ((site[1] + rx) & 1)
        f[iy, ix] = 144
        gpu_pipe.set_debayer_method("mht")
        assert_images_equal(gpu_pipe.process(f, pattern), mht_reference(f, pattern), "impulse %s %s %dx%d" % (pattern, site, w, h))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_flat_colours_come_back(gpu_pipe, pattern):
    gpu_pipe.set_debayer_method("mht")
    for h, w in ((3, 3), (4, 5), (5, 7), (64, 48), (130, 260)):
        img = np.empty((h, w, 3), np.uint8)
        img[:] = (17, 230, 96)
        assert_images_equal(gpu_pipe.process(synth.mosaic(img, pattern), pattern), img, "flat %s %dx%d" % (pattern, h, w))


def test_batch_with_padded_rows_on_the_device(gpu_pipe):
    """apply_device over frames whose rows are wider than the image (pitch not a multiple of 4) and 180 degrees."""
    import torch
    w, h, n = 301, 66, 3
    frames = np.stack([synth.gen_frame(w, h, "bayer_gbrg8", seed=40 + i, kind="uniform") for i in range(n)])
    wide = torch.zeros((n, h, w + 6), dtype=torch.uint8, device="cuda")
    wide[:, :, :w] = torch.from_numpy(frames).cuda()
    configure(gpu_pipe, flip_cfg(180))
    gpu_pipe.set_debayer_method("mht")
    out = gpu_pipe.apply_device(wide[:, :, :w], "bayer_gbrg8")
    torch.cuda.synchronize()
    for i in range(n):
        assert_images_equal(out[i].cpu().numpy(), flip(mht_reference(frames[i], "bayer_gbrg8"), 180), "frame %d" % i)


def batch_against_reference(gpu_pipe, w, h, n, pattern, angle, seed, what):
    """n different frames as one resident batch, demosaic and flip only; every frame against the flipped numpy restatement."""
    import torch
    frames = np.stack([synth.gen_frame(w, h, pattern, seed=seed + i, kind="uniform" if i % 2 else "scene") for i in range(n)])
    assert len({f.tobytes() for f in frames}) == n
    configure(gpu_pipe, flip_cfg(angle))
    gpu_pipe.set_debayer_method("mht")
    ow, oh = (h, w) if angle in (90, 270) else (w, h)
    out = torch.full((n, oh, ow, 3), 0x5A, dtype=torch.uint8, device="cuda")  # a pixel nobody writes must not pass on recycled memory
    gpu_pipe.apply_device(torch.from_numpy(frames).cuda(), pattern, out=out)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for i in range(n):
        assert_images_equal(out[i], flip(mht_reference(frames[i], pattern), angle), "%s frame %d/%d" % (what, i, n))


@pytest.mark.parametrize("angle", ANGLES)
@pytest.mark.parametrize("n", [4, 5, 8, 9, 13])
@pytest.mark.parametrize("size", [(328, 200), (645, 483)])
def test_frame_groups(gpu_pipe, size, n, angle):
    """The tile kernel takes four frames per workgroup visit: ceil(n / 4) frame groups, a workgroup of group g walks frames
    g, g + groups, ... and prefetches the next one of ITS group into registers on interior tiles.  n = 5: frames 0 2 4 / 1 3
    (uneven groups); 8: two even groups; 9 and 13: three and four groups, the last frame alone in its stride.  328 x 200 has
    6 x 7 tiles with interior ones and aligned dword stores, 645 x 483 stores bytes."""
    w, h = size
    pattern = PATTERNS[(n + angle // 90) % 4]
    batch_against_reference(gpu_pipe, w, h, n, pattern, angle, 500 + 20 * n, "groups %s n %d %s flip %d" % (size, n, pattern, angle))


TILE_EDGE_SIZES = [(w, h) for w in (61, 63, 64, 65, 67, 68, 127, 129, 132) for h in (31, 32, 33, 34, 63, 65)]


@pytest.mark.parametrize("angle", ANGLES)
@pytest.mark.parametrize("size", TILE_EDGE_SIZES)
def test_tile_edges(gpu_pipe, size, angle):
    """Widths and heights around one and two 64 x 32 tiles: partial last tiles of 1 to 4 columns / rows, the reflect-101 halo
    inside a tile next to the edge tile, dword stores that depend on cols % 4 (flip 180) and rows % 4 (flip 90), the
    quarter turns' transposed tile whose first destination column is negative on the last partial tile."""
    w, h = size
    pattern = PATTERNS[TILE_EDGE_SIZES.index(size) % 4]
    batch_against_reference(gpu_pipe, w, h, 2, pattern, angle, 700 + w + h, "edges %s %s flip %d" % (size, pattern, angle))


# ---- the full chain: MHT handle vs a bgr8 handle fed the MHT images -----------------------------------------------------
def chain_cfg(w, h, wb_method, **kw):
    base = dict(flip=True, flip_angle=180, wb=True, wb_method=wb_method, wb_temporal=wb_method == "ccc", cc=True, gamma=True,
                gamma_k=0.8, vig=True, ce=True, ce_sat=1.2, undistort=True, cam=synth.camera_model(w, h))
    base.update(kw)
    return cfg(**base)


def twin_pair(c, ccc=False):
    """(MHT handle on Bayer frames, bilinear handle that will be fed the MHT images as bgr8), both configured by c."""
    pipes = []
    for method in ("mht", "bilinear"):
        p = new_pipe(method)
        configure(p, c)
        if ccc:
            p.set_ccc_model(*synth.ccc_model())
        pipes.append(p)
    return pipes


@pytest.mark.parametrize("fp_contract", [0, 1])
@pytest.mark.parametrize("wb_method", ["grey_world", "pca", "simple", "ccc"])
def test_full_chain_batch_2448x2048(rip_lib, wb_method, fp_contract):
    import torch
    w, h, n = 2448, 2048, 3 if wb_method == "ccc" else 2
    pattern = "bayer_rggb8"
    c = chain_cfg(w, h, wb_method)
    mht_pipe, bgr_pipe = twin_pair(c, ccc=wb_method == "ccc")
    for p in (mht_pipe, bgr_pipe):
        p.set_fp_contraction(fp_contract)
    tints = [(0.70, 1.00, 0.55), (0.55, 1.00, 0.80), (0.90, 0.95, 0.50)]
    frames = np.stack([synth.gen_frame(w, h, pattern, seed=60 + i, kind="scene", tint=tints[i]) for i in range(n)])
    images = np.stack([mht_reference(frames[i], pattern) for i in range(n)])
    with mht_pipe.launch_log() as log:
        got = mht_pipe.apply_device(torch.from_numpy(frames).cuda(), pattern)
    want = bgr_pipe.apply_device(torch.from_numpy(images).cuda(), "bgr8")
    torch.cuda.synchronize()
    # the tile kernel writes the flipped MHT image, the colour chain (Lab + HSV stage set, 512 threads) of the chosen model and
    # the ring remap follow; nothing falls back to a generic kernel
    mode = {"grey_world": 1, "ccc": 2, "pca": 3, "simple": 4}[wb_method]
    assert_launched(log, ["demosaic_mht_tile_kernel<0, 0, 180>", "chain_color_kernel<15, %d, 512>" % mode, "remap_ring_kernel<?, 3, false>"],
                    GENERIC_KERNELS, "MHT full chain %s" % wb_method)
    assert ("chain_color_kernel<15, %d, 512>" % mode, fp_contract) in log.keys(), log.text
    assert got.shape == want.shape
    for i in range(n):
        assert_images_equal(got[i].cpu().numpy(), want[i].cpu().numpy(), "%s fc%d frame %d" % (wb_method, fp_contract, i))
    if wb_method == "ccc":
        assert np.array_equal(mht_pipe.get_ccc_track(n), bgr_pipe.get_ccc_track(n))


@pytest.mark.parametrize("angle", [0, 90, 180])
def test_taps_through_apply_submit_and_submit_to(rip_lib, angle):
    from raw_image_pipeline_amd.pipeline import host_alloc
    w, h = 320, 240
    pattern = "bayer_grbg8"
    c = chain_cfg(w, h, "grey_world", flip_angle=angle, cam=synth.camera_model(h, w) if angle == 90 else synth.camera_model(w, h))
    mht_pipe, bgr_pipe = twin_pair(c)
    frames = [synth.gen_frame(w, h, pattern, seed=80 + i, kind="scene") for i in range(3)]
    for f in frames:
        img = mht_reference(f, pattern)
        want = bgr_pipe.process(img, "bgr8")
        want_col = bgr_pipe.get_dist_color_image()
        want_deb = flip(img, angle)
        assert_images_equal(bgr_pipe.get_dist_debayered_image(), want_deb, "bgr8 twin's debayered tap")
        # rip_apply
        assert_images_equal(mht_pipe.process(f, pattern), want, "apply final")
        assert_images_equal(mht_pipe.get_dist_debayered_image(), want_deb, "apply debayered tap")
        assert_images_equal(mht_pipe.get_dist_color_image(), want_col, "apply colour tap")
        # rip_submit / rip_collect, taps downloaded with the result
        mht_pipe.set_tap_download(3)
        t = mht_pipe.submit(f, pattern)
        assert_images_equal(mht_pipe.collect(t), want, "submit final")
        assert_images_equal(mht_pipe.get_dist_debayered_image(), want_deb, "submit debayered tap")
        assert_images_equal(mht_pipe.get_dist_color_image(), want_col, "submit colour tap")
        # rip_submit_to into page-locked arrays of the caller
        out = host_alloc(want.shape)
        tap_d = host_alloc(want_deb.shape)
        tap_c = host_alloc(want_col.shape)
        t = mht_pipe.submit(f, pattern, out=out, tap_debayered=tap_d, tap_color=tap_c)
        mht_pipe.collect(t)
        assert_images_equal(out, want, "submit_to final")
        assert_images_equal(tap_d, want_deb, "submit_to debayered tap")
        assert_images_equal(tap_c, want_col, "submit_to colour tap")


def test_debug_dumps(rip_lib, tmp_path, monkeypatch):
    w, h = 160, 120
    pattern = "bayer_bggr8"
    c = chain_cfg(w, h, "pca", flip_angle=180)
    dirs = {}
    pipes = {}
    for method in ("mht", "bilinear"):
        d = tmp_path / method
        d.mkdir()
        monkeypatch.setenv("RIP_DEBUG_DIR", str(d))  # read when the handle is created
        pipes[method] = new_pipe(method)
        configure(pipes[method], c)
        pipes[method].set_debug(True)
        dirs[method] = d
    frame = synth.gen_frame(w, h, pattern, seed=90, kind="scene")
    img = mht_reference(frame, pattern)
    pipes["mht"].process(frame, pattern)
    pipes["bilinear"].process(img, "bgr8")
    assert_images_equal(read_png(str(dirs["mht"] / "00_debayer.png")), normalize_minmax(img), "00_debayer: before the flip")
    assert_images_equal(read_png(str(dirs["mht"] / "01_flip.png")), normalize_minmax(flip(img, 180)), "01_flip: after it")
    for name in DUMP_NAMES:
        assert_images_equal(read_png(str(dirs["mht"] / (name + ".png"))), read_png(str(dirs["bilinear"] / (name + ".png"))), name)


@pytest.mark.parametrize("angle", ANGLES)
@pytest.mark.parametrize("encoding", ["bayer_rggb16", "bayer_bggr16", "bayer_gbrg16", "bayer_grbg16"])
def test_16bit_extension(gpu_pipe, encoding, angle):
    w, h = 131, 67
    rng = np.random.default_rng(angle + len(encoding))
    frame = rng.integers(0, 65536, (h, w), dtype=np.uint16)
    frame[10:30, 20:60] = 65535  # saturated block: the clamp at 65535 is reached
    frame[40:50, 70:90] = 0      # and the one at 0
    gpu_pipe.set_debayer_16bit(True)
    configure(gpu_pipe, flip_cfg(angle))
    gpu_pipe.set_debayer_method("mht")
    got = gpu_pipe.process(frame, encoding)
    assert got.dtype == np.uint16 and gpu_pipe.last_encoding == "bgr16"
    ref = flip(mht_reference(frame, encoding), angle)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), "max |diff| %d" % int(np.abs(got.astype(np.int64) - ref).max())


def test_switching_methods_on_one_handle(rip_lib):
    w, h = 320, 240
    pattern = "bayer_rggb8"
    c = chain_cfg(w, h, "grey_world")
    frames = [synth.gen_frame(w, h, pattern, seed=100 + i, kind="scene") for i in range(2)]

    def fresh(method):
        p = new_pipe(method)
        configure(p, c)
        return p

    p = fresh("bilinear")
    for method in ("bilinear", "mht", "bilinear"):
        p.set_debayer_method(method)
        q = fresh(method)
        for f in frames:
            assert_images_equal(p.process(f, pattern), q.process(f, pattern), "switched to %s" % method)


def test_mht_differs_from_bilinear_on_a_scene(gpu_pipe):
    frame = synth.gen_frame(320, 240, "bayer_rggb8", seed=3, kind="scene")
    gpu_pipe.set_debayer_method("bilinear")
    bil = gpu_pipe.process(frame, "bayer_rggb8")
    gpu_pipe.set_debayer_method("mht")
    mht = gpu_pipe.process(frame, "bayer_rggb8")
    assert_images_equal(mht, mht_reference(frame, "bayer_rggb8"), "mht")
    assert (bil != mht).mean() > 0.05


def test_mht_launch_counts_as_chain(gpu_pipe):
    import torch
    frames = torch.from_numpy(np.stack([synth.gen_frame(256, 128, "bayer_rggb8", seed=s) for s in range(4)])).cuda()
    gpu_pipe.set_debayer_method("mht")
    gpu_pipe.apply_device(frames, "bayer_rggb8")
    torch.cuda.synchronize()
    gpu_pipe.profile_begin(16)
    gpu_pipe.apply_device(frames, "bayer_rggb8")
    launches = {k: n for k, (_, n) in gpu_pipe.profile_end().items()}
    assert sorted(launches.values()) == [0, 0, 0, 2], launches  # the MHT pass and the chain on its image, one class
    assert launches[gpu_pipe.KERNEL_CLASSES[2]] == 2, launches
