"""The covariances of the C++ mirror header's PoseGraph (include/icp_mi355x.hpp: marginalCovariance,
jointMarginalCovariance, relativeCovariance, closureDistance): tests/cpp/pose_graph_marginals_demo.cpp must compile
cleanly.  Runs on the CPU (no device needed)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pose_graph_marginals_demo_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pose_graph_marginals_demo.cpp")])
