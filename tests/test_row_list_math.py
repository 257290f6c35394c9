"""Host check of the packed row list's index arithmetic (csrc/list_reuse.h): tests/cpp/row_list_check.cpp, built with the
host compiler, forms the list of the rows listed again from random masks the way k_row_list does (densities 0, 1e-4,
1 %, 50 % and 1; row counts that are no multiple of 64) and wants exactly the ascending indices of the set bits and
their count."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_list_is_the_set_bits_in_ascending_order(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "row_list_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "row_list_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 45 "), r.stdout
