"""Host check of the pose graph's information factors (csrc/pose_graph_info_host.h, the functions behind
icpmi_information_from_icp and the checks of icpmi_pose_graph_add_*_information): tests/cpp/pose_graph_info_check.cpp,
built with the host compiler, runs every refusal -- a sigma or floor that is not allowed, a non-finite entry; a matrix
that is not finite, not symmetric, indefinite, or semi-definite without a floor -- and this file then holds the Python
restatement (scripts/pose_graph_info_ref.py) to the library's bits through the same program.  No GPU: both functions
are pure host code."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import pose_graph_info_ref as I  # noqa: E402
import pose_graph_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("pg_info") / "pose_graph_info_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "pose_graph_info_check.cpp"), "-o", exe], check=True)
    return exe


def test_every_refusal_and_the_factorisation(check_exe):
    r = subprocess.run([check_exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout


def _run(exe, mode, values):
    r = subprocess.run([exe, mode] + [float(v).hex() for v in values], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split()


def test_restatement_has_the_librarys_bits(check_exe):
    rng = np.random.default_rng(11)
    for case in range(6):
        A = rng.normal(size=(40, 6)) * np.array([3.0, 3.0, 3.0, 1.0, 1.0, 1.0])
        JtJ = A.T @ A
        T = R.se3_exp(np.r_[rng.normal(0, 0.8, 3), rng.normal(0, 5.0, 3)])
        sigma, fr, ft = [(0.02, 0.0, 0.0), (0.05, 0.5, 0.0), (1.0, 0.0, 2.0), (0.3, 0.1, 1.0), (0.02, 0.0, 0.0),
                         (7.0, 1.0, 10.0)][case]
        out = _run(check_exe, "info", list(JtJ.ravel()) + list(T.ravel()) + [sigma, fr, ft])
        got = np.array([float.fromhex(v) for v in out]).reshape(6, 6)
        want = I.information_from_icp(JtJ, T, sigma, fr, ft)
        assert np.array_equal(got, want) and np.array_equal(got, got.T)
        out = _run(check_exe, "chol", list(got.ravel()))
        assert out[0] == "0"
        tri = np.array([float.fromhex(v) for v in out[1:]])
        assert np.array_equal(tri, I.cholesky_upper(want)[np.triu_indices(6)])
    # ... and a refusal comes back as one from both
    out = _run(check_exe, "chol", list((-np.eye(6)).ravel()))
    assert out == ["3"]
    with pytest.raises(R.PoseGraphError):
        I.cholesky_upper(-np.eye(6))
