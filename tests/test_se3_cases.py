"""tests/golden/se3_cases.npz (scripts/make_se3_cases.py), the yardstick of tests/test_gpu_se3.py: it regenerates to the
committed bytes, the CPU restatement meets the errors recorded in it, its cases reach every branch and both sides of
every seam of csrc/se3.h, and the check program compiles for gfx950."""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import make_se3_cases as M  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "se3_cases.npz")


@pytest.fixture(scope="module")
def fx():
    return M.load(GOLDEN)


def test_regenerates_to_the_committed_bytes(tmp_path):
    out = tmp_path / "se3_cases.npz"
    M.save(str(out), M.make())
    assert out.read_bytes() == open(GOLDEN, "rb").read()
    assert os.path.getsize(GOLDEN) < 100 * 1024


def test_restatement_meets_its_recorded_errors(fx):
    ce = M.class_errors(fx, M.case_errors(fx, M.restatement(fx)))
    for m in ("coefs",) + M.PARTS:
        assert (ce[m] <= fx["err_" + m]).all(), m
    # what the bounds of the device test rest on: a few eps everywhere, but for the coefficients that cancel above 0.1
    assert fx["err_exp"].max() <= 9e-16 and fx["err_log"].max() <= 9e-16 and fx["err_relog"].max() <= 9e-16
    assert fx["err_jr"][:, 0].max() <= 2e-15 and fx["err_jr"][:, 1].max() <= 2e-14
    assert max(fx["err_" + m].max() for m in ("inv", "mul", "adj")) <= 4 * np.finfo(np.float64).eps
    assert fx["err_coefs"][:, :2].max() <= 4 * np.finfo(np.float64).eps
    names = list(fx["class_names"])
    assert 1e-11 < fx["err_coefs"][names.index("small"), 4:].min() and fx["err_coefs"][:, 4:].max() < 2e-10


def _quat(T12):
    """se3.h's so3_log up to the quaternion: (branch, w before the flip, |q_v| and w after it)."""
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = T12[:9]
    tr = r00 + r11 + r22
    if tr >= r00 and tr >= r11 and tr >= r22:
        br, w = 0, 0.5 * math.sqrt(1.0 + tr)
        f = 0.25 / w
        q = ((r21 - r12) * f, (r02 - r20) * f, (r10 - r01) * f)
    elif r00 >= r11 and r00 >= r22:
        x = 0.5 * math.sqrt(1.0 + r00 - r11 - r22)
        f = 0.25 / x
        br, w, q = 1, (r21 - r12) * f, (x, (r01 + r10) * f, (r02 + r20) * f)
    elif r11 >= r22:
        y = 0.5 * math.sqrt(1.0 - r00 + r11 - r22)
        f = 0.25 / y
        br, w, q = 2, (r02 - r20) * f, ((r01 + r10) * f, y, (r12 + r21) * f)
    else:
        z = 0.5 * math.sqrt(1.0 - r00 - r11 + r22)
        f = 0.25 / z
        br, w, q = 3, (r10 - r01) * f, ((r02 + r20) * f, (r12 + r21) * f, z)
    return br, w, math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), abs(w)


def test_cases_reach_every_branch_and_seam(fx):
    xi, pose, cases = fx["xi"], fx["pose"], fx["cases"]
    names = list(fx["class_names"])
    assert len(names) == 27 and 150 <= len(xi) <= 400
    # the angle the maps see: sqrt(x x + y y + z z) in se3.h's order
    th = np.sqrt(xi[:, 0] * xi[:, 0] + xi[:, 1] * xi[:, 1] + xi[:, 2] * xi[:, 2])
    for seam in (1e-8, 0.1):
        for side in (th < seam, th >= seam):
            assert side.sum() >= 6
        # the seam value itself and both neighbours, exactly (axis-aligned axes)
        for v in (np.nextafter(seam, 0.0), seam, np.nextafter(seam, 1.0)):
            assert (th == v).sum() >= 2, (seam, v)
    assert (th == 0.0).sum() >= 6 and ((th > 0) & (th < 1e-11)).sum() >= 6
    q = [_quat(p) for p in pose]
    br = np.array([b for b, _, _, _ in q])
    for b in range(4):
        assert (br == b).sum() >= 6, b
    # each branch on both sides of its seam: axis-aligned at pi/2, (1,1,1) at 2 pi/3, and with ties above
    for lo, hi, axes_ in (("pi/2-", "pi/2+", range(6)), ("2pi/3-", "2pi/3+", (M.AXIS_111,))):
        for a in axes_:
            k_lo = np.flatnonzero((cases[:, 0] == names.index(lo)) & (cases[:, 1] == a))
            k_hi = np.flatnonzero((cases[:, 0] == names.index(hi)) & (cases[:, 1] == a))
            assert len(k_lo) == 1 and len(k_hi) == 1
            assert br[k_lo[0]] == 0 and br[k_hi[0]] != 0, (lo, a)
    hi_axis = {br[k] for k in range(len(br)) if cases[k, 1] < 6 and cases[k, 0] == names.index("pi/2+")}
    assert hi_axis == {1, 2, 3}
    for a, tied in ((M.AXIS_110, (1, 2)), (M.AXIS_101, (1, 3))):
        k = np.flatnonzero((cases[:, 1] == a) & (fx["theta"] >= 2.0) & (fx["theta"] < 3.2))
        assert len(k) >= 7 and all(br[i] in tied for i in k), a
    flip = np.array([w < 0.0 for _, w, _, _ in q])
    assert flip.sum() >= 6 and set(br[flip]) == {1, 2, 3}            # the w < 0 flip, in each branch that can have it
    # 3.5 flips unless the largest axis component is negative; 5.0 wraps to 1.28 about the opposite axis: w branch
    assert flip[cases[:, 0] == names.index("3.5")].sum() >= 6
    assert (br[cases[:, 0] == names.index("5.0")] == 0).all()
    s_over_w = np.array([s < 1e-6 * w for _, _, s, w in q])
    for c, want in (("1.9e-6", True), ("2.1e-6", False), ("1e-5", False), ("1e-12", True)):
        assert (s_over_w[cases[:, 0] == names.index(c)] == want).all(), c
    assert (th > np.pi - 2e-9).sum() >= 6 and (th[th < 3.2] <= np.pi).all()
    # axes and translations
    A = fx["axes"]
    assert A.shape == (27, 3) and np.allclose(np.linalg.norm(A, axis=1), 1.0, atol=1e-15)
    assert set(cases[:, 1]) == set(range(27)) and set(cases[:, 2]) == set(range(6))
    for c in range(27):
        assert set(cases[cases[:, 0] == c, 2]) == set(range(6)), names[c]
    vmax = np.abs(xi[:, 3:]).max(axis=1)
    assert (vmax[cases[:, 2] == 0] == 0).all() and (vmax[cases[:, 2] == 5] > 100).all()
    # the pairs for inverse / compose / adjoint
    sub = fx["subset"]
    assert len(sub) >= 40 and (fx["partner"][sub] != sub).all()
    assert len(set(cases[sub, 0])) == 27


def test_check_program_compiles_for_gfx950(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc"),
                           os.path.join(ROOT, "scripts", "micro", "se3_check.hip"), "-o", str(tmp_path / "se3_check")],
                          stderr=subprocess.DEVNULL)
    assert os.path.getsize(tmp_path / "se3_check") > 0
