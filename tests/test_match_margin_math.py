"""Host check of the match margin (csrc/list_reuse.h: list_cover, match_margin, match_certified):
tests/cpp/match_margin_check.cpp, built with the host compiler, models a registration's passes and requires that every
row the margin certifies keeps the fp64 brute force's nearest neighbour -- and that rows on exact ties or against a
duplicated target never certify, while a settled uniform registration certifies at least half of its rows."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_certified_rows_keep_the_nearest_neighbour(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "match_margin_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "match_margin_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "1500"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout
