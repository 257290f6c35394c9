"""Host check of the pose graph's relative covariance and closure distance (csrc/pose_graph_marginals_host.h, the
functions behind icpmi_pose_graph_relative_covariance and icpmi_pose_graph_closure_distance):
tests/cpp/pose_graph_marginals_check.cpp, built with the host compiler, runs cases with a known answer and every
refusal; this file then holds the header to the Python restatement (scripts/pose_graph_marginals_ref.py) on random
inputs through the same program.  No GPU: both functions are pure host code.

Tolerances: both sides form the same sums of at most 12 products (relative covariance) in fp64 in different orders,
so an entry differs by at most gamma_26 ~ 2.9e-15 times the sum of the products' magnitudes, |J| |Sigma| |J|^T, formed
below.  d^2 = e^T M^-1 e: a Cholesky solve of a 6 x 6 with condition kappa has relative error of order 6^2 kappa eps."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import pose_graph_marginals_ref as M  # noqa: E402
import pose_graph_ref as R  # noqa: E402

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("pg_marg") / "pose_graph_marginals_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "pose_graph_marginals_check.cpp"), "-o", exe], check=True)
    return exe


def test_known_answers_and_every_refusal(check_exe):
    r = subprocess.run([check_exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout


def _run(exe, mode, values):
    r = subprocess.run([exe, mode] + [float(v).hex() for v in values], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split()


def _spd(rng, n, scale):
    A = rng.normal(size=(n, n + 4))
    d = scale * np.exp(rng.normal(0, 1.0, n))
    return (A @ A.T) * np.outer(d, d)


def test_header_agrees_with_the_restatement(check_exe):
    rng = np.random.default_rng(14)
    for case in range(8):
        Xi = R.se3_exp(np.r_[rng.normal(0, 1.0, 3), rng.normal(0, 20.0, 3)])
        Xj = Xi @ R.se3_exp(np.r_[rng.normal(0, 0.7, 3), rng.normal(0, 5.0, 3)])
        joint = _spd(rng, 12, 0.01)
        out = _run(check_exe, "rel", list(Xi.ravel()) + list(Xj.ravel()) + list(joint.ravel()))
        got = np.array([float.fromhex(v) for v in out]).reshape(6, 6)
        want = M.relative_covariance(Xi, Xj, joint)
        Ja = np.abs(np.hstack([R.adjoint(R.inverse(Xj) @ Xi), np.eye(6)]))
        bound = 64 * EPS * (Ja @ np.abs(joint) @ Ja.T)       # gamma_26 on each side, and the adjoint's own rounding
        assert (np.abs(got - want) <= bound).all(), (case, np.abs(got - want).max())
        assert np.array_equal(got, got.T)
        Z = R.inverse(Xi) @ Xj @ R.se3_exp(np.r_[rng.normal(0, 0.02, 3), rng.normal(0, 0.1, 3)])
        edge = _spd(rng, 6, 0.01)
        out = _run(check_exe, "dist", list(Xi.ravel()) + list(Xj.ravel()) + list(Z.ravel()) + list(want.ravel())
                   + list(edge.ravel()))
        assert out[0] == "1"
        d2 = float.fromhex(out[1])
        ref = M.closure_distance(Xi, Xj, Z, want, edge)
        kappa = np.linalg.cond(want + edge)
        # the residual e itself is a difference of poses of size ~20 m: its entries carry ~1e-15 * 20 of rounding
        e = R.se3_log(R.inverse(Z) @ (R.inverse(Xi) @ Xj))
        de = 64 * EPS * (1.0 + np.abs(Xi[:3, 3]).max() + np.abs(Xj[:3, 3]).max())
        slack = 2.0 * np.abs(np.linalg.solve(want + edge, e)).sum() * de
        print("case %d d2 %.6g ref %.6g kappa %.3g" % (case, d2, ref, kappa))
        assert abs(d2 - ref) <= 100 * kappa * EPS * ref + slack
    # a sum that is not positive definite is refused
    out = _run(check_exe, "dist", list(np.eye(4).ravel()) * 3 + list(np.eye(6).ravel()) + list((-np.eye(6)).ravel()))
    assert out[0] == "0"
