"""Host check of the registration loop's plan (csrc/loop_plan.h: make_loop_plan, fuse_step, fuse_finish, lean_next):
tests/cpp/loop_plan_check.cpp, built with the host compiler, holds them to the flat chain of conditions they replaced on
every edge of the sizes they look at and every combination of rule, engine and switches, asserts the implications between
the plan's fields and compares the lean passes' bookkeeping pass by pass.  No GPU: which form a call takes is data."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_matches_the_flat_derivation(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "loop_plan_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "loop_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout
