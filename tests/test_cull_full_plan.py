"""Host check of the plan's culled full passes (csrc/loop_plan.h: LoopPlan::cull_full): tests/cpp/cull_full_plan_check.cpp,
built with the host compiler, holds the field to its condition written out flat on the edges of the window of target sizes
(12 and 13 splits, kCullMaxSplits and one more), of the row limits (sorted rows from 4,096; 2^25), and for every switch, rule
and engine; asserts what the field implies of the others and that its switch moves no other field.  Built once plainly and
once with the address and undefined-behaviour sanitizers.  No GPU: which form a call takes is data."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_cull_full_matches_its_condition(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "cull_full_plan_check")
    subprocess.run([cxx] + flags + ["-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc"),
                                    os.path.join(ROOT, "tests", "cpp", "cull_full_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout
