"""The header-only C++ facade (include/raw_image_pipeline/raw_image_pipeline.hpp) compiles as C++14
against the C-ABI library and behaves like the reference class for a caller."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "facade_test.cpp")


# "stand-in": the facade's own raw_image_pipeline::Mat (-DRIP_NO_OPENCV); "cv": the cv::Mat branch a ROS / pybind11 workspace
# takes, compiled against tests/cpp/fake_opencv (OpenCV itself is not installable here)
BRANCHES = {"stand-in": ["-DRIP_NO_OPENCV"], "cv": ["-I", os.path.join(ROOT, "tests", "cpp", "fake_opencv")]}


def build_facade_test(tmp_path, rip_lib, branch="stand-in"):
    exe = str(tmp_path / ("facade_test_" + branch.replace("-", "_")))
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror"] + BRANCHES[branch] + ["-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_env(device):
    env = dict(os.environ)
    env["RIP_DEVICE"] = str(device)
    # the standalone binary uses ROCm's HIP runtime (no torch in the process)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return env


@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade_compiles_and_handles_parameters(tmp_path, rip_lib, branch):
    exe = build_facade_test(tmp_path, rip_lib, branch)
    r = subprocess.run([exe, "host"], capture_output=True, text=True, env=run_env(-1))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "facade host OK" in r.stdout and "no CPU execution path" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_facade_apply_matches_oracle(tmp_path, rip_lib, oracle, branch):
    from helpers import cfg, oracle_run
    exe = build_facade_test(tmp_path, rip_lib, branch)
    w, h = 64, 48
    out_path = str(tmp_path / "out.bin")
    r = subprocess.run([exe, "gpu", str(w), str(h), out_path], capture_output=True, text=True, env=run_env(0))
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out_path, np.uint8).reshape(h, w, 3)
    s = 12345
    vals = []
    for _ in range(w * h):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        vals.append(s >> 24)
    frame = np.array(vals, np.uint8).reshape(h, w)
    c = cfg(flip=True, flip_angle=180, wb=True, wb_method="gray_world", wb_bright=0.8, cc=True,
            cc_matrix=[1.5, -0.25, 0.0, 0.125, 1.0, -0.125, 0.0, -0.5, 1.75], cc_bias=(1.0, -2.0, 3.5), gamma=True, gamma_k=0.8, vig=True)
    ref, _ = oracle_run(oracle, c, frame, "bayer_rggb8")
    assert np.array_equal(got, ref)


RIG_SRC = os.path.join(ROOT, "examples", "camera_rig.cpp")


def build_rig_example(tmp_path, branch):
    exe = str(tmp_path / ("camera_rig_" + branch.replace("-", "_")))
    libdir = os.path.join(ROOT, "raw_image_pipeline_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror"] + BRANCHES[branch] + ["-I", os.path.join(ROOT, "include"), RIG_SRC, "-o", exe,
           "-L", libdir, "-l:librip_hip.so", "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined", "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_camera_rig_example_compiles_and_refuses_to_run_without_a_device(tmp_path, rip_lib, branch):
    """examples/camera_rig.cpp (include/raw_image_pipeline/camera_rig.hpp: one handle per camera, camera c on devices[c % n],
    cameras overlapped with submit / collect from one thread, worker threads as an option) builds as C++14 on both Mat branches; without a HIP device it fails loudly."""
    import torch
    exe = build_rig_example(tmp_path, branch)
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the gpu-marked test runs the example")
    r = subprocess.run([exe, "2", "64", "48", "1", str(tmp_path / "rig_"), "0"], capture_output=True, text=True, env=run_env(0))
    assert r.returncode == 1 and "no CPU execution path" in r.stdout


@pytest.mark.gpu
def test_camera_rig_example_two_cameras_on_device_0_match_oracle(tmp_path, rip_lib, oracle):
    """Two cameras with different parameters (gamma, white-balance method) on device 0 through the C++ rig, overlapped with
    submit / collect from one thread and once more from one worker thread each (the example compares the two itself): the
    last frame of each camera equals the oracle's result for that camera's configuration."""
    from helpers import cfg, oracle_run
    exe = build_rig_example(tmp_path, "stand-in")
    w, h, n_frames = 96, 64, 5
    prefix = str(tmp_path / "rig_")
    r = subprocess.run([exe, "2", str(w), str(h), str(n_frames), prefix, "0"], capture_output=True, text=True, env=run_env(0))
    assert r.returncode == 0 and "camera rig OK" in r.stdout, r.stdout + r.stderr
    for c in range(2):
        s = (1000 * c + (n_frames - 1) + 1) & 0xFFFFFFFF
        vals = []
        for _ in range(w * h):
            s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
            vals.append(s >> 24)
        frame = np.array(vals, np.uint8).reshape(h, w)
        conf = cfg(flip=True, flip_angle=180, wb=True, wb_method="pca" if c % 2 else "gray_world", wb_bright=0.8, cc=True,
                   cc_matrix=[1.5, -0.25, 0.0, 0.125, 1.0, -0.125, 0.0, -0.5, 1.75], gamma=True, gamma_k=0.7 + 0.05 * c, vig=True)
        ref, _ = oracle_run(oracle, conf, frame, "bayer_rggb8")
        got = np.fromfile(prefix + "%d.bin" % c, np.uint8).reshape(h, w, 3)
        assert np.array_equal(got, ref), "camera %d" % c
