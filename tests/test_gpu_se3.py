"""The device SE(3) maps (csrc/se3.h: se3_coefs, se3_exp, se3_log, se3_jr_inv, se3_inv, se3_mul, se3_adjoint) one thread per
case (scripts/micro/se3_check.hip) against the 60-digit results of tests/golden/se3_cases.npz
(scripts/make_se3_cases.py): 188 twists over 27 angles -- 0, the seams at 1e-8, 2e-6 and 0.1 with their fp64 neighbours,
the Shepperd seams at pi/2 and 2 pi/3, up to pi - 1e-9, and 3.5 and 5.0 whose log wraps -- general, tied and axis-aligned
axes, translations up to 1e3.

Allowed error, per map, output part and angle class: 8 x the error of the fp64 CPU restatement (scripts/pose_graph_ref.py)
recorded in the fixture, at least 8 eps.  The device evaluates the same formulas in the same order and can differ only in
the last bits of sin, cos, atan2 and sqrt, which pass through the same cancellation as the restatement's.  Rotation
parts are absolute; translation-carrying parts (v of exp and log, the coupling block of Jr^-1, t^ R of the adjoint, t of
inverse and compose) are divided by 1 + |v|_inf; the raw coefficients are relative.  Above pi - 1e-6 the sign of the
log's axis is not determined by the rounded pose: there the device's log is put through the restatement's exp and
compared with the pose, under the same rule.

Measured on an MI355X, largest error of the device / of the restatement, and the largest device error over allowed error:
    coefs  8.87e-11 / 8.87e-11 (E and F just above 0.1, relative; A and B <= 2.4e-16)   0.250
    exp    6.66e-16 / 6.66e-16    0.250        log    8.88e-16 / 4.44e-16    0.250
    jr     1.38e-14 / 1.38e-14 (coupling block at pi - 1e-6, |v| ~ 1e3; Jw^-1 block 1.6e-15)   0.170
    inv    1.49e-16 / 1.49e-16    0.084        mul    1.68e-16 / 1.20e-16    0.094        adj    1.49e-16 / 1.27e-16    0.084
The restatement's errors per angle class are in the fixture (err_*); a host build of se3.h with glibc's libm gives the
restatement's figures to the digit."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import make_se3_cases as M  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
MARGIN = 8.0
MAPS = ("coefs", "exp", "log", "jr", "inv", "mul", "adj")
BELOW_TINY = ("0", "1e-12", "9.9e-9", "tiny-")          # classes with theta < kSe3Tiny
SIGN_FREE = ("pi-1e-9",)                                # classes with theta > pi - 1e-6


def ratios(fx, got):
    """Per map: (largest error / allowed error over cases and parts, where, largest device error, the restatement's)."""
    errs = M.case_errors(fx, got)
    cls = fx["cases"][:, 0]
    names = list(fx["class_names"])
    free = np.isin(cls, [names.index(c) for c in SIGN_FREE])
    out = {}
    for m in MAPS:
        e = errs[m]
        k = cls if len(e) == len(cls) else cls[fx["subset"]]
        allowed = np.maximum(MARGIN * fx["err_" + m][k], MARGIN * EPS)
        r = e / allowed
        rec = fx["err_" + m].max()
        if m == "log":
            f = free[:, None] & np.ones_like(r, dtype=bool)
            r = np.where(f, errs["relog"] / np.maximum(MARGIN * fx["err_relog"][k], MARGIN * EPS), r)
            e = np.where(f, errs["relog"], e)
        assert np.isfinite(r).all(), (m, "not finite")
        w = np.unravel_index(np.argmax(r), r.shape)
        out[m] = (float(r[w]), (names[k[w[0]]], int(w[0]), int(w[1])), float(e.max()), float(rec))
    return out


@pytest.fixture(scope="module")
def fx():
    return M.load(os.path.join(ROOT, "tests", "golden", "se3_cases.npz"))


@pytest.fixture(scope="module")
def device(fx, tmp_path_factory):
    """Compile the check program with the library's flags and run it once."""
    tmp = tmp_path_factory.mktemp("se3")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, fin, fout = tmp / "se3_check", tmp / "cases.f64", tmp / "results.f64"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc"),
                           os.path.join(ROOT, "scripts", "micro", "se3_check.hip"), "-o", str(exe)],
                          stderr=subprocess.DEVNULL)
    M.pack(fx).tofile(str(fin))
    out = subprocess.run(["timeout", "-k", "10", "120", str(exe), str(fin), str(fout)], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    got = M.unpack(fx, np.fromfile(str(fout), dtype=np.float64))
    return got, ratios(fx, got)


@pytest.mark.parametrize("m", MAPS)
def test_map_against_60_digits(device, m):
    ratio, where, dev, ref = device[1][m]
    print("se3 %-5s device/allowed %.3f at %s; largest error device %.3g, restatement %.3g" % (m, ratio, where, dev, ref))
    assert ratio <= 1.0, (m, ratio, where)


def test_jr_inv_blocks(device):
    """The upper right block is zero and the lower right one is the upper left one, exactly."""
    J = device[0]["jr6"]
    assert (J[:, :3, 3:] == 0.0).all()
    assert (J[:, 3:, 3:] == J[:, :3, :3]).all()


def test_log_of_identity_is_zero(fx, device):
    eye = (fx["pose"] == np.r_[np.eye(3).ravel(), 0, 0, 0]).all(axis=1)
    assert eye.sum() >= 1
    assert (device[0]["log"][eye] == 0.0).all()


def test_below_tiny_series_values(fx, device):
    """0 <= theta < 1e-8: finite, and the coefficients are the series values (their theta^2 terms round away)."""
    names = list(fx["class_names"])
    sel = np.isin(fx["cases"][:, 0], [names.index(c) for c in BELOW_TINY])
    assert sel.sum() >= 4 * 6 and (fx["theta"][sel] < 1e-8).all()
    got = device[0]
    assert (got["coefs"][sel] == np.array([1.0, 0.5, 1.0 / 6, 1.0 / 12, 1.0 / 24, 1.0 / 120])).all()
    for m in ("exp", "log", "jr6"):
        assert np.isfinite(got[m][sel]).all()


def _series(th):
    """C, D, E, F below kSe3Small as se3.h writes them: only + - * /, so fp64 gives the same bits anywhere."""
    t2 = th * th
    return np.stack([1.0 / 6 - t2 * (1.0 / 120 - t2 * (1.0 / 5040 - t2 * (1.0 / 362880 - t2 / 39916800))),
                     1.0 / 12 + t2 * (1.0 / 720 + t2 * (1.0 / 30240 + t2 * (1.0 / 1209600 + t2 / 47900160))),
                     1.0 / 24 - t2 * (1.0 / 720 - t2 * (1.0 / 40320 - t2 * (1.0 / 3628800 - t2 / 479001600))),
                     1.0 / 120 - t2 * (1.0 / 2520 - t2 * (1.0 / 120960 - t2 * (1.0 / 9979200 - t2 / 1245404160)))], -1)


def test_series_below_small_and_closed_forms_from_it(fx, device):
    """theta < 0.1 gives the series' bits; theta = 0.1 and its upper neighbours give the closed forms, whose E and F lose
    seven digits there and so cannot equal the series' bits (which an accuracy bound alone would prefer)."""
    th, got = fx["theta"], device[0]["coefs"]
    s = _series(th)
    lo = th < 0.1
    assert lo.sum() >= 60 and (got[lo, 2:] == s[lo]).all()
    names = list(fx["class_names"])
    at = np.isin(fx["cases"][:, 0], [names.index(c) for c in ("small", "small+", "0.1000001")])
    assert at.sum() >= 18 and (th[at] >= 0.1).all()
    assert (got[at, 4] != s[at, 2]).all() and (got[at, 5] != s[at, 3]).all()
