"""Host check of solo passes as data (csrc/loop_plan.h: LoopPlan::solo_on, solo_next): tests/cpp/solo_plan_check.cpp, built
with the host compiler, holds the plan's field to its condition written out flat on both edges of every term (65,472 /
65,473 and 131,072 / 131,073 rows, profile levels 1 and 2, every switch, rule and engine), checks that the switch and the
test hook move nothing else, holds solo_next to a slow restatement over random count sequences, and asserts that a solo
tail implies a lean pass behind it.  Built once plainly and once with the address and undefined-behaviour sanitizers.
No GPU: which form a call takes is data."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_solo_plan_matches_its_condition(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "solo_plan_check")
    subprocess.run([cxx] + flags + ["-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc"),
                                    os.path.join(ROOT, "tests", "cpp", "solo_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout
