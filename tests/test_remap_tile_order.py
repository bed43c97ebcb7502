"""The order in which the ring remap kernels visit their tiles (csrc/rip_tile_deal.hpp), walked on the host: every run length and
order enumerates every tile exactly once.  No GPU."""
import subprocess

import pytest

from helpers import build_host_program


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_every_order_and_run_length_visits_every_tile_exactly_once(tmp_path, sanitize):
    """tests/cpp/tile_deal_test.cpp: TileDeal and tile_deal_geometry compiled as host code through the HIP host stub, the tile loop
    of the ring kernels restated for every workgroup of six grid sizes.  Geometries: one tile (64 x 16), 200 x 72 (a partial last
    tile column, 4.5 tile rows: the last run is shorter than the strip), 328 x 144 (9 tile rows: one full run of 8 and a ragged one,
    XCDs without work), the sizes of the GPU suite, the three benchmark sizes 2448 x 2048, 1920 x 1200, 3840 x 2160, and the widest
    and the highest plan the launchers accept.  Run lengths 0 (contiguous) to 2^20 tile rows, orders row-major, column strips, column strips
    where they deal out evenly, and an unknown one.  The second build adds -fsanitize=address,undefined to this stand-alone program."""
    exe = build_host_program(tmp_path, "tile_deal_test", ["tile_deal_test.cpp"], sanitize=sanitize, extra=["-Wall", "-Werror"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "3696 cases, 0 bad" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
