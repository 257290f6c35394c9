"""Host check of list reuse's certificate (csrc/list_reuse.h): tests/cpp/list_reuse_check.cpp, built with the host
compiler, keeps a row's list only where an fp64 brute force finds the row's nearest neighbour inside it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kept_lists_hold_the_nearest_neighbour(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "list_reuse_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "list_reuse_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "40000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
