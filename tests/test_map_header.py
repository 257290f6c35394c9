"""The global-map part of the C++ mirror header (include/icp_mi355x.hpp): tests/cpp/map_demo.cpp, the node's
run_pose_graph_optimization -> rebuild_recent_clouds and build_final_global_map -> rebuild_occupancy_grid ->
publish_global_map with the mirror behind them, must compile cleanly.  Runs on the CPU (no device needed)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_map_demo_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "map_demo.cpp")])
