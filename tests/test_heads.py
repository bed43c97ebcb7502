"""Output heads (include/rip.h rip_set_output_heads, rip_select_output_head, rip_apply_device_heads, rip_apply_heads) without a GPU:
defaults, setters and getters per head, shrinking, index and range refusals, every query under every selection against a twin handle
that holds that head alone, the YAML sections, the C++ facade, the refusal order of the heads calls as far as it is decided without a
device, the build, and head_copy_kernel of csrc/rip_heads.hip executed on the host -- plainly and under AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program.  Everything at tolerance 0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import heads_cases as HC
from helpers import build_host_program
from raw_image_pipeline_amd import RawImagePipeline
from raw_image_pipeline_amd import pipeline as P
from test_cpp_facade import BRANCHES, run_env
from test_resize import write_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = P.RIP_ERR_INVALID_ARGUMENT


def host_twin(frame, head):
    """A RIP_DEVICE_NONE handle with the frame's pipeline settings whose only output has `head`'s settings."""
    t = RawImagePipeline(False, "", "", "", device=-1)
    HC.configure_pipeline(t, frame)
    HC.apply_head(t, head)
    return t


# ---- heads, selection, setters -----------------------------------------------------------------------------------------------
def test_defaults(host_pipe):
    p = host_pipe
    assert p.get_output_heads() == 1 and p.get_selected_output_head() == 0
    assert HC.read_head(p) == HC.DEFAULT
    assert P.RIP_OK == 0 and hasattr(p._lib, "rip_apply_heads")


def test_setters_and_getters_per_head_do_not_leak(host_pipe):
    p = host_pipe
    heads = HC.BY_NAME["eight"].heads
    HC.configure_heads(p, heads)
    assert p.get_output_heads() == 8 and p.get_selected_output_head() == 0
    for k in (3, 0, 7, 1, 6, 2, 5, 4):
        p.select_output_head(k)
        assert p.get_selected_output_head() == k and HC.read_head(p) == heads[k], k
    # one head rewritten: the others keep theirs
    p.select_output_head(4)
    HC.apply_head(p, HC.CROP_CUBIC)
    for k in range(8):
        p.select_output_head(k)
        assert HC.read_head(p) == (HC.CROP_CUBIC if k == 4 else heads[k]), k


def test_shrinking_resets_the_removed_heads_and_the_selection(host_pipe):
    p = host_pipe
    heads = HC.BY_NAME["mean_upscale_aa"].heads
    HC.configure_heads(p, heads)
    p.select_output_head(3)
    p.set_output_heads(2)
    assert p.get_output_heads() == 2 and p.get_selected_output_head() == 0
    p.select_output_head(1)
    assert HC.read_head(p) == heads[1]
    p.set_output_heads(2)                                   # the same n: nothing changes, the selection stays
    assert p.get_selected_output_head() == 1 and HC.read_head(p) == heads[1]
    p.set_output_heads(4)
    assert p.get_selected_output_head() == 1
    for k in (2, 3):
        p.select_output_head(k)
        assert HC.read_head(p) == HC.DEFAULT, k
    p.select_output_head(0)
    assert HC.read_head(p) == heads[0]


def test_index_and_range_refusals(host_pipe):
    p = host_pipe
    for n in (0, -1, 9, 1 << 30):
        with pytest.raises(ValueError, match="1..8"):
            p.set_output_heads(n)
    assert p.get_output_heads() == 1
    for k in (1, -1, 8):
        with pytest.raises(ValueError, match=r"heads 0\.\.0"):
            p.select_output_head(k)
    p.set_output_heads(3)
    p.select_output_head(2)
    with pytest.raises(ValueError, match=r"heads 0\.\.2"):
        p.select_output_head(3)
    assert p.get_selected_output_head() == 2
    with pytest.raises(ValueError):
        p.debug_output_head_info(3)
    assert p.debug_output_head_info(2) == (0, 0, 0)
    lib = p._lib
    assert lib.rip_get_output_heads(p._h, None) == P.RIP_OK and lib.rip_get_selected_output_head(p._h, None) == P.RIP_OK
    assert lib.rip_set_output_heads(None, 2) == INVALID and lib.rip_select_output_head(None, 0) == INVALID


@pytest.mark.parametrize("head_set", HC.SETS, ids=HC.set_id)
def test_queries_under_each_selection_equal_the_twins(host_pipe, head_set):
    """rip_query_output, rip_query_output_bytes, rip_get_output_camera_info and rip_get_output_window under each selected head equal
    those of a twin handle configured with that head alone (floats compared with ==)."""
    p = host_pipe
    f = HC.FRAMES[head_set.frame]
    HC.configure_pipeline(p, head_set.frame)
    HC.configure_heads(p, head_set.heads)
    geometry = (f.size[1], f.size[0], f.channels, f.encoding)
    for k in reversed(range(len(head_set.heads))):
        t = host_twin(head_set.frame, head_set.heads[k])
        p.select_output_head(k)
        for call in ("query_output", "query_output_bytes", "get_output_window"):
            assert getattr(p, call)(*geometry) == getattr(t, call)(*geometry), (k, call)
        got, want = p.get_output_camera_info(*geometry), t.get_output_camera_info(*geometry)
        assert got[:2] == want[:2] and all(np.array_equal(a, b) for a, b in zip(got[2:], want[2:])), k


def test_a_query_refusal_belongs_to_the_selected_head_alone(host_pipe):
    p = host_pipe
    HC.configure_pipeline(p, "bayer136")
    HC.configure_heads(p, (HC.IDENTITY, HC.Head(size=(300, 100), interp="area"), HC.CROP_CUBIC))
    geometry = (72, 136, 1, "bayer_rggb8")
    assert p.query_output(*geometry)[:3] == (72, 136, 3)
    p.select_output_head(1)
    with pytest.raises(ValueError):
        p.query_output(*geometry)          # area refuses the upscale
    p.select_output_head(2)
    assert p.query_output(*geometry) == (64, 96, 3, "rgb8")


# ---- YAML --------------------------------------------------------------------------------------------------------------------
def test_yaml_sections_in_any_order_and_with_gaps(tmp_path, host_pipe):
    p = host_pipe
    p.load_params(write_params(tmp_path, "output_3:\n  size: [50, 40]\n  interpolation: linear_aa\n  format: bgr_chw_bf16\n"
                                         "output:\n  format: rgb8\n"
                                         "output_1:\n  roi: [8, 4, 64, 32]\n  format: mono8\n  pad: [1, 2, 3]\n"))
    assert p.get_output_heads() == 4 and p.get_selected_output_head() == 0
    assert p._output_format == "rgb8" == p.get_output_format()
    want = {0: HC.Head(format="rgb8"), 1: HC.Head(format="mono8", roi=(8, 4, 64, 32), pad=(1, 2, 3)), 2: HC.DEFAULT,
            3: HC.Head(format="bgr_chw_bf16", size=(50, 40), interp="linear_aa")}
    for k, h in want.items():
        p.select_output_head(k)
        assert HC.read_head(p) == h, k
    # a file without such a section: one head, as before there were heads; the selection goes back to 0
    p.load_params(write_params(tmp_path, "output:\n  size: [64, 48]\n"))
    assert p.get_output_heads() == 1 and p.get_selected_output_head() == 0 and p.get_output_size() == (64, 48)
    p.load_params(write_params(tmp_path, "output_7:\n  fit: crop\n"))
    assert p.get_output_heads() == 8
    p.select_output_head(7)
    assert p.get_output_fit() == "crop"
    p.load_params(write_params(tmp_path, "debayer:\n  enabled: true\n"))
    assert p.get_output_heads() == 1 and HC.read_head(p) == HC.DEFAULT


@pytest.mark.parametrize("bad", ["output_8:\n  format: rgb8\n", "output_12:\n  format: rgb8\n", "output_0:\n  format: rgb8\n", "output_x:\n  format: rgb8\n",
                                 "output_2:\n  format: rgb9\n", "output_2:\n  size: [0, 5]\n", "output_1:\n  fit: fill\n", "output_5:\n  pad: [0, 0, 256]\n",
                                 "output_1:\n  roi: [0, 0, 4]\n", "output_3:\n  interpolation: cubic\n", "output_1:\n  std: [1, 0, 1]\n"])
def test_yaml_invalid_section_fails_and_changes_nothing(tmp_path, host_pipe, bad):
    p = host_pipe
    heads = (HC.CROP_CUBIC, HC.WINDOW_MONO)
    HC.configure_heads(p, heads)
    p.select_output_head(1)
    p.set_flip(True)
    with pytest.raises(ValueError):
        p.load_params(write_params(tmp_path, "output:\n  format: rgb8\n%sflip:\n  enabled: false\n" % bad))
    assert p.get_output_heads() == 2 and p.get_selected_output_head() == 1 and p.is_flip_enabled()
    for k in (0, 1):
        p.select_output_head(k)
        assert HC.read_head(p) == heads[k]


def test_a_bad_value_in_a_section_is_named_with_its_section(tmp_path, host_pipe):
    with pytest.raises(ValueError, match="output_2: size"):
        host_pipe.load_params(write_params(tmp_path, "output_2:\n  size: [1, 2, 3]\n"))
    with pytest.raises(ValueError, match="output: size"):
        host_pipe.load_params(write_params(tmp_path, "output:\n  size: [1, 2, 3]\n"))


# ---- the heads calls, as far as they are decided without a device --------------------------------------------------------------
def heads_call(p, d_in=1, heads=True, encoding=b"bayer_rggb8", n_heads=None, requested=(0,), n_frames=1, rows=72, cols=136):
    n = p.get_output_heads() if n_heads is None else n_heads
    bufs = (P._HeadBuffer * max(n, 1))()
    for k in requested:
        bufs[k] = P._HeadBuffer(C.c_void_p(4096), 0, 0)
    st = p._lib.rip_apply_device_heads(p._h, C.c_void_p(d_in), C.c_size_t(0), C.c_size_t(0), n_frames, rows, cols, 1, encoding,
                                       bufs if heads else None, n, None, None)
    return st, p._lib.rip_last_error(p._h).decode()


def test_the_heads_calls_need_a_device_first(host_pipe):
    st, msg = heads_call(host_pipe)
    assert st == P.RIP_ERR_DEVICE and "RIP_DEVICE_NONE" in msg
    outs, caps = (C.c_void_p * 1)(), (C.c_size_t * 1)()
    st = host_pipe._lib.rip_apply_heads(host_pipe._h, C.c_void_p(4096), 72, 136, 1, C.c_size_t(0), b"bayer_rggb8", outs, caps, 1, None, None, None)
    assert st == P.RIP_ERR_DEVICE
    with pytest.raises(P.RipError):
        host_pipe.apply_heads(np.zeros((72, 136), np.uint8), "bayer_rggb8")
    assert host_pipe._lib.rip_apply_device_heads(None, None, C.c_size_t(0), C.c_size_t(0), 1, 72, 136, 1, b"bayer_rggb8", None, 1, None, None) == INVALID


def test_python_refuses_heads_outside_the_handle(host_pipe):
    host_pipe.set_output_heads(2)
    for heads in ([], [2], [-1], [0, 5]):
        with pytest.raises(ValueError, match=r"0\.\.1"):
            host_pipe.apply_heads(np.zeros((72, 136), np.uint8), "bayer_rggb8", heads=heads)


def test_python_names_the_head_whose_settings_refuse_the_frame(host_pipe):
    p = host_pipe
    HC.configure_pipeline(p, "bayer136")
    HC.configure_heads(p, (HC.IDENTITY, HC.Head(size=(300, 100), interp="area")))
    p.select_output_head(1)
    with pytest.raises(ValueError, match="^output head 1: "):
        p.apply_heads(np.zeros((72, 136), np.uint8), "bayer_rggb8")
    assert p.get_selected_output_head() == 1      # put back


# ---- the facade ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade(tmp_path, rip_lib, branch):
    exe = str(tmp_path / ("heads_test_" + branch.replace("-", "_")))
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror"] + BRANCHES[branch] + ["-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "heads_test.cpp"), "-o", exe, "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir,
           "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=run_env(-1))
    assert r.returncode == 0 and "heads host OK" in r.stdout, r.stdout + r.stderr


# ---- the kernel on the host ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_kernel_run_on_the_host_copies_every_byte_and_no_other(tmp_path, sanitize):
    """tests/cpp/heads_kernel_host.cpp: csrc/rip_heads.hip compiled as host code with the toolchain's clang++, every thread of the
    launcher's grid run in turn from an exactly sized staging image into an exactly sized destination: row lengths 1 .. 70 and 4095 ..
    4098 bytes, destination phases 0 .. 17, three pitches, 1 and 3 frames; every byte compared, sentinels everywhere else.  The second
    build adds -fsanitize=address,undefined to this stand-alone program: no access outside either block, no misaligned wide access."""
    exe = build_host_program(tmp_path, "heads_kernel_host", ["heads_kernel_host.cpp"], sanitize=sanitize, extra=["-ffp-contract=off", "-Wall"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "7992 cases, 0 bad" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
