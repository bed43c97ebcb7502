"""The host units below the handle stand on their own (csrc/rip_yaml.cpp, rip_params.cpp, rip_output_tables.cpp): a stand-alone program
links these three and nothing else of the library, without any HIP header or library.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_yaml_params_and_output_tables_link_and_work_without_the_rest(tmp_path, sanitize):
    """tests/cpp/host_units_test.cpp: a parameter text with an `output:` and an `output_2:` section is loaded and read back field by
    field; every check function of a setting gets one refused value, directly and through a parameter text, and the refused load
    leaves Modules as it was; output_window_geometry is compared with a letterbox and a crop case worked out by hand.  The second
    build adds -fsanitize=address,undefined to this stand-alone program."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    cpp, csrc = os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "raw_image_pipeline_amd", "csrc")
    exe = str(tmp_path / "host_units_test")
    units = [os.path.join(csrc, u) for u in ("rip_yaml.cpp", "rip_params.cpp", "rip_output_tables.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off"] + san + ["-I", csrc, os.path.join(cpp, "host_units_test.cpp")] + units + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(tmp_path / "params.yaml")], capture_output=True, text=True)
    assert r.returncode == 0 and "49 checks, 0 bad" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
