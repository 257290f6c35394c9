"""Host check of the lean-pass rule (csrc/list_reuse.h: lean_pass, lean_schedule): tests/cpp/lean_rule_check.cpp, built with
the host compiler, runs the rule on count sequences -- never zero; zero from pass 3; zero, zero, then non-zero; alternating;
zeros only in a call's first passes; calls of 1, 2 and 3 passes -- against the lean passes written down by hand."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lean_rule_on_count_sequences(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "lean_rule_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "lean_rule_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout
