"""Host test of select_apply_transpose_part (sem_amd/csrc/apply_select.h), the selection of
sem_apply_transpose_part: every handle kind, the element-position range of the handle's own columns, the
one algo, the order range, the offset limit on the local vector and the order of those checks.

tests/host/apply_select_part_main.cpp is a stand-alone program over the header alone, built with the host
compiler and its address and undefined-behaviour sanitizers and run as a child process; no library is loaded
and no GPU is needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_apply_select_part_policy(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("the host test of apply_select.h needs g++")
    exe = str(tmp_path / "apply_select_part_main")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "host", "apply_select_part_main.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
