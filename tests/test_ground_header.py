"""The ground-segmentation part of the C++ mirror header (include/icp_mi355x.hpp): tests/cpp/ground_demo.cpp, a scan
labelled on its own and the occupancy counts built from the kept scans' OBSTACLE rows, must compile cleanly.  Runs on
the CPU (no device needed)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ground_demo_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "ground_demo.cpp")])
