"""Host test of the band kernel's division-free tile map (sem_amd/csrc/band_tile_map.h).

tests/host/band_tile_map_main.cpp is a stand-alone program over the header alone: the multiply-high split against
/ and % (every tiles_y in 1..4096 with every L < 2^20; every tiles_y below the derived bound 2^26 at the multiples
of tiles_y and their neighbours up to the launcher's tile limit), and the whole blockIdx -> (tx, ty) map, XCD remap
included, as a bijection onto the tile grid.  It is built with the host compiler and its address and
undefined-behaviour sanitizers and run as a child process; no library is loaded and no GPU is needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_band_tile_map(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("the host test of band_tile_map.h needs g++")
    exe = str(tmp_path / "band_tile_map_main")
    subprocess.run([cxx, "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "host", "band_tile_map_main.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
