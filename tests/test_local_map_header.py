"""The local-map part of the C++ mirror header (include/icp_mi355x.hpp): tests/cpp/local_map_demo.cpp, scan-to-local-map
odometry with the mirror behind it, must compile cleanly.  Runs on the CPU (no device needed)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_local_map_demo_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "local_map_demo.cpp")])
