"""Host check of the context's buffer layouts (csrc/workspace_layout.h: MiscBlock, SortPlanes, BoundedRows, KnnRows,
GroupCounters, PartialRows, ProgressRings): tests/cpp/workspace_layout_check.cpp, built with the host compiler, holds every
layout to the hand-written offsets and sizes it replaced, offset for offset and byte for byte on the edges of the sizes they
look at, and asserts that each layout's members ascend, do not overlap, end within its bytes and are aligned as their
readers need.  No GPU: where things lie in a buffer is data."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layouts_match_the_hand_written_offsets(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "workspace_layout_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "workspace_layout_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout
