"""The information edges of the C++ mirror header (include/icp_mi355x.hpp: last_normal_matrix, information_from_icp,
PoseGraph::addOdometryInformation / addLoopClosureInformation, LoopClosureConfig::information_sigma):
tests/cpp/pose_graph_info_demo.cpp must compile cleanly.  Runs on the CPU (no device needed)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pose_graph_info_demo_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pose_graph_info_demo.cpp")])
