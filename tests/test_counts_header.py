"""The hit / miss count part of the C++ mirror header (include/icp_mi355x.hpp): tests/cpp/counts_demo.cpp, the node's
cells_to_occupancy_grid_msg publishing GlobalMap::raycast_counts' probability, must compile cleanly.  Runs on the CPU
(no device needed)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_counts_demo_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "counts_demo.cpp")])
