"""Host check of the live count plane's growth arithmetic (csrc/live_plane.h): tests/cpp/live_plane_check.cpp, built with
the host compiler, feeds live_plane_grow the windows of straight, diagonal, spiral and random-walk drives at R = 0, 40,
200 and 4096, from cells of both signs and next to +-(2^31 - 2 - R - 6), and checks after every step that the new box
holds the old box and the window, that only crossed sides moved, that the cells copied so far are at most 4 x the
box's, and that nothing the planner accepts is refused; then the two spans at 2^31 - 1 cells."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_growth_keeps_its_four_conditions(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "live_plane_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "live_plane_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 80 drives"), r.stdout
