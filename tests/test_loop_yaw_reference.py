"""Loop closures on revisits with another heading, on the CPU: scripts/loop_yaw_ref.py, the restatement of
Scan Context's distance with its argmin kept and of the detector that starts each verification from it, against the
oracle; icpmi_sc_shift_transform (host only) against the restatement; and the Python mirror's yaw_guess with the
oracle behind it on the fixed drives R12 (a street driven back facing the other way), H12 (one place, twelve headings)
and D78 (the node's whole loop: out, turn round, back).  No device needed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import loop_yaw_ref as ref  # noqa: E402
from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402
from lidar_slam_from_scratch_amd import loop_closure as lc  # noqa: E402

# What the guess has to beat by construction: half a voxel and half a sector.
TOL_M, TOL_RAD = 0.25, np.radians(3.0)

R12_CFG = dict(frame_gap=50, sc_distance_threshold=0.2, icp_fitness_threshold=0.3)
H12_CFG = dict(frame_gap=1, sc_distance_threshold=0.25, icp_fitness_threshold=0.3, max_candidates=10)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def r12():
    poses, labels = ref.r12_reverse_drive()
    return poses, labels, ref.scans(poses)


@pytest.fixture(scope="module")
def h12():
    poses, labels = ref.h12_headings()
    return poses, labels, ref.scans(poses)


def _tie_descriptor():
    """period 30 sectors, small integers: every sum is exact, and shifts s and s + 30 give the same distance"""
    half = np.random.default_rng(5).integers(0, 8, (20, 30)).astype(np.float64)
    return np.concatenate([half, half], axis=1)


# ---------------------------------------------------------------------------------------------------------------- the shift

def test_min_of_shift_distances_is_the_oracles_distance(oracle, r12):
    descs = [oracle.scan_context(c) for c in r12[2]]
    for a in descs[6:]:
        for b in descs[:6]:
            d = ref.shift_distances(a, b)
            assert d.shape == (60,)
            assert _bits([d.min()]) == _bits([oracle.scan_context_distance(a, b)])
            assert _bits([ref.distance_shift(a, b)[0]]) == _bits([d.min()])


def test_best_shift_recovers_every_roll(oracle, r12):
    D = oracle.scan_context(r12[2][0])
    for s in range(60):
        assert ref.best_shift(np.roll(D, -s, axis=1), D) == s


def test_tie_goes_to_the_smaller_shift():
    P = _tie_descriptor()
    for s in range(60):
        d = ref.shift_distances(np.roll(P, -s, axis=1), P)
        assert _bits([d[s % 30]]) == _bits([d[s % 30 + 30]])
        assert ref.best_shift(np.roll(P, -s, axis=1), P) == s % 30


def test_zero_descriptor(oracle, r12):
    D = oracle.scan_context(r12[2][0])
    Z = np.zeros((20, 60))
    assert ref.distance_shift(Z, D) == (1.0, 0) and ref.distance_shift(D, Z) == (1.0, 0)


def test_shift_transform_is_the_librarys():
    from lidar_slam_from_scratch_amd import build
    build.build_library()
    lib = capi.load_library()
    for s in range(60):
        T = np.full((4, 4), np.nan)
        assert lib.icpmi_sc_shift_transform(s, capi._dp(T)) == capi.OK
        assert np.array_equal(_bits(T), _bits(ref.shift_transform(s))), s
        assert np.array_equal(_bits(lc.sc_shift_transform(s)), _bits(T))
    assert np.array_equal(_bits(ref.shift_transform(0)), _bits(np.eye(4)))
    a = np.radians(6.0 * 17)
    assert np.allclose(ref.shift_transform(17)[:2, :2], [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]], atol=1e-15)
    T = np.zeros((4, 4))
    for bad in (-1, 60):
        assert lib.icpmi_sc_shift_transform(bad, capi._dp(T)) == capi.ERR_ARG
        with pytest.raises(ValueError):
            ref.shift_transform(bad)
    assert not T.any()


# ---------------------------------------------------------------------------------------------------------------- the detector

def _drive_detect(clouds, labels, cfg, backend, every=True):
    det = lc.LoopClosureDetector(backend, cfg)
    found = []
    for k, (c, label) in enumerate(zip(clouds, labels)):
        det.add_frame(c, label)
        if every or k == len(clouds) - 1:
            found += det.detect()
    return found


def _errors(found, poses, labels):
    at = {label: i for i, label in enumerate(labels)}
    return [synth.pose_delta(np.asarray(r.transform), ref.truth(poses, at[r.query_frame], at[r.match_frame])) for r in found]


def test_r12_reverse_drive(oracle, r12):
    poses, labels, clouds = r12
    off_backend = ref.OracleBackend(oracle)
    off = _drive_detect(clouds, labels, lc.LoopClosureConfig(**R12_CFG), off_backend)
    assert len(off_backend.iterations) == 11 and off == []           # every candidate verified from the identity: none holds
    on = _drive_detect(clouds, labels, lc.LoopClosureConfig(yaw_guess=True, **R12_CFG), ref.OracleBackend(oracle))
    assert len(on) == 9
    first = {}
    for r in on:
        first.setdefault(r.query_frame, r)
    assert [(q, first[q].match_frame, first[q].sector_shift) for q in range(100, 106)] == \
        [(100, 5, 28), (101, 4, 28), (102, 3, 29), (103, 2, 29), (104, 1, 30), (105, 0, 30)]
    firsts = [first[q] for q in range(100, 106)]
    print("R12 first results: fitness", [r.icp_fitness for r in firsts], "errors", _errors(firsts, poses, labels))
    for r, (dt, dr) in zip(firsts, _errors(firsts, poses, labels)):
        assert r.icp_fitness < 0.3 and dt <= TOL_M and dr <= TOL_RAD
    # the restatement's detector: the same closures, bit for bit
    yd = ref.YawLoopClosureDetector(ref.OracleBackend(oracle), lc.LoopClosureConfig(yaw_guess=True, **R12_CFG))
    again = []
    for c, label in zip(clouds, labels):
        yd.add_frame(c, label)
        again += yd.detect()
    assert [(r.query_frame, r.match_frame, r.sector_shift) for r in again] == \
        [(r.query_frame, r.match_frame, r.sector_shift) for r in on]
    for x, y in zip(again, on):
        assert _bits([x.scan_context_distance, x.icp_fitness]).tolist() == _bits([y.scan_context_distance, y.icp_fitness]).tolist()
        assert np.array_equal(_bits(x.transform), _bits(y.transform))


def test_h12_twelve_headings(oracle, h12):
    poses, labels, clouds = h12
    off = _drive_detect(clouds, labels, lc.LoopClosureConfig(**H12_CFG), ref.OracleBackend(oracle), every=False)
    on = _drive_detect(clouds, labels, lc.LoopClosureConfig(yaw_guess=True, **H12_CFG), ref.OracleBackend(oracle), every=False)
    assert len(on) == 10 and len(off) < 10
    assert len({r.sector_shift for r in on}) == 10
    assert all(r.sector_shift is None for r in off)
    print("H12 errors", _errors(on, poses, labels))
    for dt, dr in _errors(on, poses, labels):
        assert dt <= TOL_M and dr <= TOL_RAD


def test_backend_without_the_keywords_still_works_when_off(oracle, r12):
    """a backend with today's four-argument align and no distances_shift"""
    class Plain:
        def scan_context(self, cloud):
            return oracle.scan_context(cloud)

        def distances(self, q, hist):
            return np.array([oracle.scan_context_distance(q, h) for h in hist])

        def align(self, s, t, mi, tol):
            return oracle.icp_point_to_plane(s, t, mi, tol, 1e-9)

    _, labels, clouds = r12
    assert _drive_detect(clouds[:7], labels[:7], lc.LoopClosureConfig(**R12_CFG), Plain()) == []


def test_d78_node_loop(oracle):
    """slam.run_slam over out - turn round - back with the oracle's ICP and the pose-graph restatement: the return leg
    closes only with the guess, and the closure takes the drift out"""
    import pose_graph_ref
    from lidar_slam_from_scratch_amd import slam
    poses = ref.d78_drive()
    frames = ref.scans(poses)
    want = np.linalg.inv(poses[0]) @ poses[-1]

    def align(s, t, mi, tol):
        return oracle.icp_point_to_plane(s, t, mi, tol, 1e-9)

    err = {}
    for on in (False, True):
        run = slam.run_slam(frames, None, align=align, loop_backend=ref.OracleBackend(oracle),
                            pose_graph=pose_graph_ref.PoseGraph(), loop_yaw_guess=on)
        assert len(run.poses) == len(frames)
        if on:
            assert any(c.query_frame == 70 and c.query_frame - c.match_frame >= 50 for c in run.closures)
            assert all(c.sector_shift is not None for c in run.closures)
        else:
            assert run.closures == []
        err[on] = synth.pose_delta(run.poses[-1], want)
    print("D78 final pose error: off", err[False], "on", err[True])
    assert err[True][0] <= 0.5 * err[False][0] and err[True][1] <= 0.5 * err[False][1]
