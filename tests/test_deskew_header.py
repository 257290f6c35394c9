"""The deskew part of the C++ mirror header (include/icp_mi355x.hpp) and the host half of the feature
(csrc/deskew_host.h).  tests/cpp/deskew_demo.cpp -- a sweep deskewed on its own, the twist of a delta, the stream
deskewing each raw scan -- must compile cleanly.  tests/cpp/deskew_host_check.cpp, a stand-alone program over
deskew_host.h, is built with the host compiler under AddressSanitizer and UBSan and run as a child process: every
refusal of the configuration check, the per-sweep constants' three forms, the log map's round trips and refusals; then
the Python restatement (scripts/deskew_ref.py) is held to the header's bits through the same program.  Runs on the CPU
(no device needed)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import deskew_ref as dr  # noqa: E402
import pose_graph_ref as R  # noqa: E402


def test_deskew_demo_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "deskew_demo.cpp")])


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("no g++")
    exe = str(tmp_path_factory.mktemp("deskew") / "deskew_host_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "deskew_host_check.cpp"), "-o", exe], check=True)
    return exe


def test_host_check_under_sanitizers(check_exe):
    r = subprocess.run([check_exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout


def _run(exe, mode, values):
    r = subprocess.run([exe, mode] + [float(v).hex() for v in values], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split()


def test_restatement_has_the_headers_bits(check_exe):
    rng = np.random.default_rng(5)
    for angle in (0.0, 3e-12, 1e-9, 2e-4, 0.03, 0.0999, 0.1001, 0.6, 2.0, 3.1):
        w = rng.normal(size=3)
        w *= angle / np.linalg.norm(w)
        xi = np.r_[w, rng.uniform(-2.0, 2.0, 3)]
        out = _run(check_exe, "twist", R.se3_exp(xi).ravel())
        got = np.array([float.fromhex(v) for v in out])
        assert np.array_equal(got, dr.twist_from_delta(R.se3_exp(xi))), angle
        out = _run(check_exe, "consts", xi)
        k = dr.constants(xi)
        want = [k["theta"]] + list(k["K"]) + list(k["K2"]) + list(k["av"]) + list(k["aav"])
        assert int(out[0]) == k["mode"], angle
        assert np.array_equal(np.array([float.fromhex(v) for v in out[1:]]), np.array(want)), angle
    assert _run(check_exe, "consts", np.zeros(6))[0] == str(dr.IDENTITY)
    bad = np.eye(4)
    bad[1, 3] = np.nan
    assert _run(check_exe, "twist", bad.ravel()) == ["refused"]
    with pytest.raises(ValueError):
        dr.twist_from_delta(bad)
