"""The yaw-guess part of the C++ mirror header (include/icp_mi355x.hpp): tests/cpp/loop_yaw_demo.cpp, both loop-closure
detectors with LoopClosureConfig::yaw_guess and LoopClosureResult::sector_shift, must compile cleanly.  Runs on the CPU
(no device needed)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_loop_yaw_demo_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "loop_yaw_demo.cpp")])
