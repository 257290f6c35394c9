"""The live count part of the C++ mirror header (include/icp_mi355x.hpp): tests/cpp/live_demo.cpp, the node's
process_frame with GlobalMap::live_update, live_counts and live_clear, must compile cleanly.  Runs on the CPU (no device
needed)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_live_demo_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "live_demo.cpp")])
