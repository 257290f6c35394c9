"""scripts/deskew_ref.py, the CPU restatement of the motion compensation (csrc/deskew.h, icpmi_deskew) that
tests/test_gpu_deskew.py holds the library to: hand-worked rows, the log map's round trips, the property the feature
rests on -- a static scene seen from a moving sensor comes back exactly -- the synthetic sweeps, and the value of it all
on a drive whose velocity changes, with the oracle as the aligner.  Runs on the CPU (no device needed)."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import deskew_ref as dr  # noqa: E402
import local_map_ref as lm  # noqa: E402
import pose_graph_ref as R  # noqa: E402
from lidar_slam_from_scratch_amd import odometry, synth  # noqa: E402

# causal ATE <= R * skewed ATE on the accelerating drive: halfway between the ratio measured once on the CPU (frame to
# frame 0.2288 m / 0.3091 m = 0.740; scan to map 0.0326 m / 0.1418 m = 0.230) and 1
R_F2F = 0.87
R_S2M = 0.615


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _rows(n, seed, extent=60.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-extent, extent, size=(n, 3)), rng.uniform(0.0, 1.0, size=n)


# ------------------------------------------------------------------ hand-worked rows
def test_zero_twist_is_the_identity_in_every_bit():
    xyz, tau = _rows(200, 1)
    xyz[:6] = [[-0.0, 0.0, -0.0], [np.nan, 1.0, 2.0], [1.0, np.inf, 2.0], [1.0, 2.0, -np.inf], [5e-324, -5e-324, 1.0], [0.0, 0.0, 0.0]]
    tau[6] = np.nan
    for t_ref in (0.0, 0.5, 1.0):
        got = dr.deskew(xyz, np.zeros(6), tau, t_ref=t_ref)
        assert np.array_equal(_bits(got.xyz), _bits(xyz))
    got = dr.deskew(xyz[7:], np.zeros(6))                              # azimuth times
    assert np.array_equal(_bits(got.xyz), _bits(xyz[7:]))


def test_pure_translation_is_p_plus_s_v_exactly():
    xyz, tau = _rows(300, 2)
    v = np.array([1.25, -0.4, 0.07])
    for w in (np.zeros(3), np.array([3e-11, -4e-11, 1e-11])):          # no rotation, and one below the tiny-angle cut
        for t_ref in (0.0, 0.5, 1.0):
            got = dr.deskew(xyz, np.r_[w, v], tau, t_ref=t_ref)
            s = tau - t_ref
            assert np.array_equal(_bits(got.xyz), _bits(xyz + s[:, None] * v[None, :]))


def test_a_row_at_t_ref_and_a_non_finite_row_pass_through():
    xyz, tau = _rows(64, 3)
    tau[:4] = 0.25
    xyz[4] = [np.nan, 1.0, 1.0]
    xyz[5] = [1.0, -np.inf, 1.0]
    tau[6], tau[7] = np.nan, np.inf
    xyz[8] = [-0.0, -0.0, -0.0]
    tau[8] = 0.25
    got = dr.deskew(xyz, [0.02, -0.01, 0.05, 1.0, 0.3, -0.2], tau, t_ref=0.25)
    assert np.array_equal(_bits(got.xyz[:9]), _bits(xyz[:9]))
    moved = np.abs(got.xyz[9:] - xyz[9:]).max(axis=1)
    assert np.all(moved > 1e-4)                                         # ... and every other row moves


def test_pure_yaw_and_a_circle_worked_by_hand():
    # the sensor turns 0.5 rad per sweep about z: a row seen at the sweep's end (tau = 1) at (1, 0, 0) lies, in the frame
    # of the sweep's start (t_ref = 0), at Exp(1 * xi) p = Rz(0.5) p = (cos 0.5, sin 0.5, 0).  Values <= 2, a handful of
    # roundings: 1e-15
    got = dr.deskew([[1.0, 0.0, 0.0], [0.0, 2.0, 1.0]], [0.0, 0.0, 0.5, 0.0, 0.0, 0.0], [1.0, 1.0], t_ref=0.0).xyz
    c, s = math.cos(0.5), math.sin(0.5)
    assert np.abs(got - [[c, s, 0.0], [-2.0 * s, 2.0 * c, 1.0]]).max() <= 1e-15
    # ... and measured at the sweep's START, registered at its END (t_ref = 1): the rotation runs backwards
    got = dr.deskew([[1.0, 0.0, 0.0]], [0.0, 0.0, 0.5, 0.0, 0.0, 0.0], [0.0], t_ref=1.0).xyz
    assert np.abs(got - [[c, -s, 0.0]]).max() <= 1e-15
    # a car on a circle of radius r = 2 turning theta = 0.5 per sweep: omega = (0, 0, theta), v = (theta r, 0, 0).  The
    # sensor's own position at the sweep's end, the origin of its frame then, lies at (r sin theta, r (1 - cos theta), 0)
    # in the frame of the start
    got = dr.deskew([[0.0, 0.0, 0.0]], [0.0, 0.0, 0.5, 1.0, 0.0, 0.0], [1.0], t_ref=0.0).xyz
    assert np.abs(got - [[2.0 * s, 2.0 * (1.0 - c), 0.0]]).max() <= 1e-15
    # from pi/4 on the library's sincos: a quarter turn
    got = dr.deskew([[3.0, 0.0, 0.0]], [0.0, 0.0, math.pi / 2, 0.0, 0.0, 0.0], [1.0], t_ref=0.0).xyz
    assert np.abs(got - [[0.0, 3.0, 0.0]]).max() <= 1e-15


def test_sincos_step_against_libm():
    a = np.r_[0.0, np.linspace(1e-12, dr.PIO4, 2000, endpoint=False), np.nextafter(dr.PIO4, 0.0), dr.PIO4, 1.0, 2.5]
    s, c = dr.sincos_step(a)
    assert np.abs(s - np.sin(a)).max() <= 2.3e-16 and np.abs(c - np.cos(a)).max() <= 2.3e-16   # below 1 ulp of values <= 1


def test_checks():
    ok = dict(twist=np.zeros(6), t_ref=0.5, time_source=dr.TIMES, direction=1, azimuth_start=-dr.PI)
    dr.check(**ok)
    for bad in (dict(twist=[0, 0, np.nan, 0, 0, 0]), dict(twist=[0, 0, 0, np.inf, 0, 0]), dict(t_ref=np.nan), dict(t_ref=-0.1),
                dict(t_ref=1.0000001), dict(time_source=2), dict(direction=0), dict(direction=2), dict(azimuth_start=np.inf)):
        with pytest.raises(ValueError):
            dr.check(**dict(ok, **bad))
    with pytest.raises(ValueError):
        dr.deskew(np.zeros((2, 3)), np.zeros(6), None, time_source=dr.TIMES)


# ------------------------------------------------------------------ the log map
def test_twist_from_delta_round_trips():
    rng = np.random.default_rng(7)
    for angle in (0.0, 1e-13, 5e-11, 9.9e-11, 1e-9, 1e-6, 1e-3, 0.02, 0.0999, 0.1001, 0.3, 0.7):   # tiny, small, moderate
        for _ in range(20):
            w = rng.normal(size=3)
            w *= angle / np.linalg.norm(w)
            xi = np.r_[w, rng.uniform(-2.0, 2.0, 3)]                     # a sweep moves a metre or two
            T = R.se3_exp(xi)
            got = dr.twist_from_delta(T)
            assert np.abs(got - xi).max() <= 1e-14, (angle, got - xi)
            assert np.abs(got - R.se3_log(T)).max() <= 1e-15, angle     # the pose graph's own log map
    assert np.array_equal(dr.twist_from_delta(np.eye(4)), np.zeros(6))


# ------------------------------------------------------------------ what the feature rests on
@pytest.mark.parametrize("t_ref", [0.0, 0.5, 1.0])
def test_a_static_scene_comes_back_exactly(t_ref):
    """World points w_i of a static scene, seen at tau_i from the pose T_ref Exp((tau_i - t_ref) xi), are the rows
    q_i = (T_ref Exp(s_i xi))^-1 w_i; deskewing q with xi returns T_ref^-1 w_i, the scene as seen from T_ref, within
    1e-12 (|w| + |v|) per coordinate: the rounding of ~50 fp64 operations with room, four orders above one ulp at 100 m."""
    rng = np.random.default_rng(11)
    for xi in ([0.0, 0.0, 0.04, 1.5, 0.0, 0.0], [0.01, -0.02, 0.05, 2.0, 0.3, -0.1], [0.0, 0.0, 0.0, 1.0, -1.0, 0.2],
               [2e-11, 0.0, 1e-11, 0.7, 0.0, 0.0], [0.2, 0.1, -0.6, 1.0, 2.0, 0.5], [0.0, 0.0, 1.4, 3.0, 0.0, 0.0]):
        xi = np.array(xi)
        T_ref = synth.make_transform(rng.normal(0.0, 0.3, 3), rng.uniform(-3.0, 3.0, 3))
        n = 400
        w = rng.uniform(-100.0, 100.0, size=(n, 3))
        tau = rng.uniform(0.0, 1.0, size=n)
        tau[:3] = [0.0, 1.0, t_ref]
        q = np.empty_like(w)
        for i in range(n):
            pose = T_ref @ dr.exp_twist(xi, tau[i] - t_ref)
            q[i] = synth.apply_transform(synth.invert_transform(pose), w[i][None, :])[0]
        got = dr.deskew(q, xi, tau, t_ref=t_ref).xyz
        want = synth.apply_transform(synth.invert_transform(T_ref), w)
        tol = 1e-12 * (np.linalg.norm(w, axis=1) + np.linalg.norm(xi[3:]))
        assert np.all(np.abs(got - want) <= tol[:, None]), np.abs(got - want).max()
        skew = np.abs(q - want).max()
        assert skew > 0.1                                                 # ... and the rows were skewed to begin with


# ------------------------------------------------------------------ synthetic sweeps
@pytest.fixture(scope="module")
def sweeps():
    """frames 0..11 of the accelerating drive at 16 x 600 as raw sweeps (rows, tau), and the true poses at t_ref"""
    return [synth.lidar_sweep(f, synth.accel_pose, beams=16, azimuths=600) for f in range(12)], [synth.accel_pose(f) for f in range(12)]


def test_the_drive_stays_inside_the_scene():
    for f in np.linspace(-0.5, 11.5, 49):
        p = synth.accel_pose(f)[:3, 3]
        assert -85.0 < p[0] < 85.0 and -30.0 < p[1] < 30.0
        assert not any(np.all(lo <= p) and np.all(p <= hi) for lo, hi in synth._scene())
    speed = [np.linalg.norm(synth.accel_pose(f + 0.5)[:3, 3] - synth.accel_pose(f - 0.5)[:3, 3]) for f in range(12)]
    assert abs(speed[0] - 0.3) < 1e-12 and abs(speed[11] - (0.3 + 0.16 * 11)) < 1e-12      # 0.3 + 0.16 frame metres per frame
    yaw = [math.degrees(math.atan2(synth.accel_pose(f)[1, 0], synth.accel_pose(f)[0, 0])) for f in range(12)]
    assert np.allclose(yaw, 0.12 * np.arange(12) ** 2, atol=1e-12)


def test_sweep_columns_are_cast_from_their_own_pose(sweeps):
    rows, tau = sweeps[0][5]
    assert rows.shape[0] == tau.shape[0] > 5000 and tau.min() >= 0.0 and tau.max() <= 1.0
    # a standing sensor's sweep is the snapshot: same rows whatever the times
    still = synth.lidar_sweep(5, lambda f: synth.accel_pose(5), beams=16, azimuths=600, range_noise=0.0)[0]
    snap = synth.lidar_sweep(5, lambda f: synth.accel_pose(5), t_ref=0.0, beams=16, azimuths=600, range_noise=0.0)[0]
    assert np.array_equal(still, snap)
    # a moving one is skewed by up to half a frame's motion at the sweep's ends
    moving = synth.lidar_sweep(5, synth.accel_pose, beams=16, azimuths=600, range_noise=0.0)
    assert moving[0].shape != still.shape or np.abs(moving[0] - still).max() > 0.3


def test_azimuth_times_equal_the_generators(sweeps):
    """tau from the rows' azimuths against the generator's, on every frame: 1e-15 (measured 2.2e-16); every beam lies half
    an azimuth step, 5.2 mrad at 600 columns, from the seam"""
    for rows, tau in sweeps[0]:
        got, margin = dr.azimuth_times(rows)
        assert margin >= 5e-3
        assert np.abs(got - tau).max() <= 1e-15
    rows, tau = sweeps[0][3]
    # clockwise, from another start: the mirrored sweep
    mirrored = rows * np.array([1.0, -1.0, 1.0])
    got, margin = dr.azimuth_times(mirrored, direction=-1, azimuth_start=dr.PI)
    assert margin >= 5e-3 and np.abs(got - tau).max() <= 1e-15


def test_the_wrap_at_the_seam():
    eps = 1e-9
    rows = np.array([[-1.0, -eps, 0.0], [-1.0, eps, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    tau, margin = dr.azimuth_times(rows)
    assert tau[0] < 1e-9 and tau[1] > 1.0 - 1e-9 and tau[2] == 0.5 and abs(tau[3] - 0.75) < 1e-15 and margin < 2e-9


# ------------------------------------------------------------------ the value of it
def _ate(track, poses):
    return odometry.absolute_trajectory_error(track, poses)


def _true_twists():
    return [dr.twist_from_delta(synth.invert_transform(synth.accel_pose(f - 0.5)) @ synth.accel_pose(f + 0.5)) for f in range(12)]


def test_deskewing_pays_on_the_accelerating_drive(sweeps):
    """Frame-to-frame and scan-to-map odometry with the oracle as aligner over the 12-frame accelerating drive at 16 x
    600, three times each: on the skewed scans, on scans deskewed with the true twist of each sweep, and on scans
    deskewed causally, with the twist of the previous frame's delta.  Measured once:
        frame to frame   skewed 0.3091 m   true twist 0.2187 m   causal 0.2288 m   (causal / skewed 0.740)
        scan to map      skewed 0.1418 m   true twist 0.0108 m   causal 0.0326 m   (causal / skewed 0.230)
    Asserted: true <= causal < skewed, and causal <= R * skewed with R halfway between the measured ratio and 1."""
    from oracle import oracle as orc
    raw, poses = sweeps
    vox = lambda p: synth.voxel_centroids(p, 0.5)  # noqa: E731
    f2f = lambda s, t, it, tol: orc.icp_point_to_plane(s, t, max_iterations=it, tolerance=tol, nthreads=4)  # noqa: E731
    s2m = lm.oracle_align(orc)
    skewed = [vox(rows) for rows, _tau in raw]
    true = [vox(dr.deskew(rows, xi, tau).xyz) for (rows, tau), xi in zip(raw, _true_twists())]
    ate = dict(f2f_skewed=_ate(odometry.run_odometry(skewed, f2f), poses), f2f_true=_ate(odometry.run_odometry(true, f2f), poses),
               f2f_causal=_ate(dr.run_odometry(raw, f2f), poses), s2m_skewed=_ate(lm.run_local_map(skewed, s2m), poses),
               s2m_true=_ate(lm.run_local_map(true, s2m), poses), s2m_causal=_ate(dr.run_local_map(raw, s2m), poses))
    print("accelerating drive, 16 x 600, 12 frames, oracle: " + "  ".join("%s %.4f m" % kv for kv in ate.items()))
    print("causal / skewed: frame to frame %.3f, scan to map %.3f" % (ate["f2f_causal"] / ate["f2f_skewed"],
                                                                      ate["s2m_causal"] / ate["s2m_skewed"]))
    assert ate["f2f_true"] <= ate["f2f_causal"] < ate["f2f_skewed"]
    assert ate["f2f_causal"] <= R_F2F * ate["f2f_skewed"]
    assert ate["s2m_true"] <= ate["s2m_causal"] < ate["s2m_skewed"]
    assert ate["s2m_causal"] <= R_S2M * ate["s2m_skewed"]

