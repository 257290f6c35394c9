"""The local map on the device: k_lmap_keys, k_lmap_marks and k_lmap_merge behind icpmi_local_map_*.  After
every add the table -- keys and points -- is byte for byte that of the CPU restatement (scripts/local_map_ref.py): scan
and resident sizes around the 64-lane and 256-thread edges, one voxel, a voxel per row, the hand-worked edge rows, poses
that evict nothing, some and everything, a rotated pose, host / device / stream-frame adds, a 12-frame drive with eviction,
the capacity error.  Registration against the table is icpmi_align*'s to the bit and the oracle's within
tests/test_gpu_parity.py's tolerances, whether the target prepared by the add is still remembered or not.  The driver
(odometry.run_odometry_local_map) in lock step with the restatement, run_slam(odom_local_map=...), the error codes."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import torch  # noqa: F401  (first: one HIP runtime per process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import local_map_ref as lm  # noqa: E402
import robust_icp_ref as rr  # noqa: E402
from lidar_slam_from_scratch_amd import capi, odometry, slam, synth  # noqa: E402
from lidar_slam_from_scratch_amd.local_map import LocalMap, LocalMapConfig  # noqa: E402
from test_gpu_parity import check_against  # noqa: E402

pytestmark = pytest.mark.gpu

I4 = np.eye(4)
SCAN_ROWS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
HUBER = (capi.ROBUST_HUBER, rr.HUBER_SCALE)


@pytest.fixture(scope="module")
def ctx():
    """Fails loudly (no skip, no fallback) when the HIP library or the device is missing."""
    from lidar_slam_from_scratch_amd import build
    build.build_library()
    c = capi.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drive16():
    """frames 0..11 of the default drive at 16 beams x 600 azimuths, and their true poses: tests/test_local_map_reference.py's"""
    return lm.drive(12, 16, 600)


def shifted(x, y=0.0, z=0.0):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return T


def rotated(yaw, pitch, t):
    T = np.eye(4)
    T[:3, :3] = synth.rotvec_to_matrix((0.0, pitch, yaw))
    T[:3, 3] = t
    return T


def _info(i):
    return dict(rows=i.rows, inserted=i.inserted, evicted=i.evicted, dropped=i.dropped, merged=i.merged)


def same_table(dev, ref):
    pts, keys = dev.points()
    assert dev.size() == ref.size() == keys.shape[0]
    assert keys.tobytes() == ref.keys.tobytes()
    assert pts.tobytes() == ref.pts.tobytes()


def add_both(dev, ref, scan, pose):
    """one add on the device and in the restatement: same counts, same bytes"""
    n, before = len(scan), ref.size()
    got, want = _info(dev.add(scan, pose)), ref.add(scan, pose)
    assert got == want
    assert got["inserted"] + got["dropped"] + got["merged"] == n and got["rows"] == before - got["evicted"] + got["inserted"]
    same_table(dev, ref)
    return got


def pair(ctx, voxel_size=0.5, max_range=100.0, capacity=1 << 14):
    return LocalMap(ctx, LocalMapConfig(voxel_size, max_range, capacity)), lm.LocalMapRef(voxel_size, max_range, capacity)


def lattice(rows):
    """`rows` points, each in a 0.5 m voxel of its own, in a block around the origin"""
    i = np.arange(rows)
    return np.stack([(i % 20) * 0.5 + 0.25 - 5.0, ((i // 20) % 20) * 0.5 + 0.25 - 5.0, (i // 400) * 0.5 + 0.25], axis=1)


# ------------------------------------------------------------------ the table's bytes
@pytest.mark.parametrize("resident", [0, 1, 256, 257, 5000])
def test_table_bytes_by_size(ctx, resident):
    """every scan size into a table of `resident` rows: the scan overlaps the residents' block, so rows are inserted,
    merged into residents and merged into each other"""
    dev, ref = pair(ctx)
    rng = np.random.default_rng(100 + resident)
    for n in SCAN_ROWS:
        dev.clear()
        ref.clear()
        if resident:
            assert add_both(dev, ref, lattice(resident), I4)["rows"] == resident
        scan = rng.uniform(-6.0, 6.0, size=(n, 3))
        info = add_both(dev, ref, scan, shifted(0.1, -0.2, 0.05))
        assert info["evicted"] == 0 and info["dropped"] == 0
        if n == 1025:
            assert info["merged"] > 0 and info["inserted"] > 0
    dev.close()


def test_one_voxel_and_a_voxel_per_row(ctx):
    dev, ref = pair(ctx)
    rng = np.random.default_rng(7)
    info = add_both(dev, ref, rng.uniform(1.01, 1.49, size=(777, 3)), I4)          # all in voxel (2, 2, 2)
    assert info == dict(rows=1, inserted=1, evicted=0, dropped=0, merged=776)
    info = add_both(dev, ref, lattice(3000)[::-1].copy(), I4)                        # keys descending: the sort's work
    assert info["inserted"] + info["merged"] == 3000 and info["merged"] <= 1
    dev.close()


def test_edge_rows(ctx):
    """tests/test_local_map_reference.py's hand-worked rows, through the kernels"""
    under_zero, under_edge = -5e-324, math.nextafter(-0.5, -math.inf)
    dev, ref = pair(ctx)
    add_both(dev, ref, np.array([[-0.0, 0.0, 0.0], [under_zero, 0.0, 1.0], [under_edge, 0.0, 2.0], [-0.5, 0.0, 3.0]]), I4)
    info = add_both(dev, ref, np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [1.0, 1.0, 1.0],
                                        [np.nan, np.nan, np.nan], [1e308, 1e308, 0.0]]), I4)
    assert info["dropped"] == 5 and info["inserted"] == 1
    dev.close()
    above = math.nextafter(10.0, math.inf)
    dev, ref = pair(ctx, max_range=10.0)
    info = add_both(dev, ref, np.array([[10.0, 0.0, 0.0], [above, 0.0, 1.0], [0.0, -10.0, 0.0], [0.0, 0.0, -above]]), I4)
    assert info == dict(rows=2, inserted=2, evicted=0, dropped=2, merged=0)
    info = add_both(dev, ref, np.array([[10.0, 0.0, 0.0], [above, 0.0, 1.0]]), shifted(100.0))
    assert info == dict(rows=1, inserted=1, evicted=2, dropped=1, merged=0)
    dev.close()
    lo, hi = -(1 << 20), (1 << 20) - 1
    dev, ref = pair(ctx, max_range=1e7)
    info = add_both(dev, ref, np.array([[lo * 0.5, 0.0, 0.0], [hi * 0.5, 0.0, 0.0], [(lo - 1) * 0.5, 0.0, 0.0],
                                        [(hi + 1) * 0.5, 0.0, 0.0], [0.0, lo * 0.5, hi * 0.5], [0.0, 0.0, (hi + 1) * 0.5],
                                        [0.0, (lo - 1) * 0.5, 0.0], [hi * 0.5, hi * 0.5, hi * 0.5], [lo * 0.5, lo * 0.5, lo * 0.5]]), I4)
    assert info == dict(rows=5, inserted=5, evicted=0, dropped=4, merged=0)
    keys = dev.points()[1]
    assert int(keys[0]) == 0 and int(keys[-1]) == (1 << 63) - 1                      # the lowest and the highest key there is
    dev.close()
    dev, ref = pair(ctx, max_range=10.0)                                             # an evicted voxel, taken again
    add_both(dev, ref, np.array([[9.9, 0.0, 0.0], [1.0, 0.0, 0.0]]), I4)
    info = add_both(dev, ref, np.array([[9.8, 0.0, 0.0]]), shifted(-0.25))
    assert info == dict(rows=2, inserted=1, evicted=1, dropped=0, merged=0)
    dev.close()


def test_eviction_and_rotation(ctx):
    dev, ref = pair(ctx, max_range=8.0)
    rng = np.random.default_rng(11)
    cloud = rng.uniform(-4.0, 4.0, size=(4000, 3))
    assert add_both(dev, ref, cloud, I4)["evicted"] == 0
    some = add_both(dev, ref, rng.uniform(-6.0, 6.0, size=(900, 3)), shifted(6.0))   # the far side leaves, the scan's corners drop
    assert 0 < some["evicted"] < some["rows"] + some["evicted"] - some["inserted"] and some["dropped"] > 0
    turned = add_both(dev, ref, rng.uniform(-4.0, 4.0, size=(1300, 3)), rotated(0.7, -0.2, (5.0, 1.0, -0.5)))
    assert turned["inserted"] > 0
    assert add_both(dev, ref, np.zeros((0, 3)), shifted(0.5))["inserted"] == 0          # n == 0: evicts only
    rows = ref.size()
    gone = add_both(dev, ref, rng.uniform(-4.0, 4.0, size=(300, 3)), shifted(1000.0))  # everything leaves
    assert gone["evicted"] == rows and gone["rows"] == gone["inserted"] > 0
    assert add_both(dev, ref, np.zeros((0, 3)), shifted(-1000.0))["rows"] == 0
    dev.close()


def test_host_device_and_stream_frame_adds_agree(ctx):
    raw = synth.lidar_frame(0, voxel=0, beams=16, azimuths=600)
    ctx.stream_reset()
    cfg = capi.Context.make_config()
    _res, _hist, info = ctx.stream_push_host(raw, 0.5, 1000, cfg)
    scan = ctx.stream_current_scan()
    assert scan.shape[0] == info.n_filtered > 1000
    pose = rotated(0.3, 0.0, (2.0, -1.0, 0.5))
    a, ref = pair(ctx)
    b, _ = pair(ctx)
    c, _ = pair(ctx)
    want = ref.add(scan, pose)
    d_scan = torch.from_numpy(scan).cuda()
    assert _info(a.add(scan, pose)) == _info(b.add_device(d_scan.data_ptr(), scan.shape[0], pose)) \
        == _info(c.add_stream_frame(pose)) == want
    for m in (a, b, c):
        same_table(m, ref)
        m.close()
    ctx.stream_reset()


def test_sequence_with_eviction(ctx, drive16):
    """twelve frames under the TRUE poses (given, not registered, so that last-bit pose differences cannot move a row
    across a voxel edge), max_range 30: the table slides"""
    frames, poses = drive16
    dev, ref = pair(ctx, max_range=30.0, capacity=1 << 16)
    evicted = 0
    for f, T in zip(frames, poses):
        evicted += add_both(dev, ref, f, T)["evicted"]
    assert evicted > 0
    dev.close()


def test_capacity(ctx):
    dev, ref = pair(ctx, max_range=10.0, capacity=3)
    add_both(dev, ref, np.array([[9.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), I4)
    with pytest.raises(capi.IcpError) as e:
        dev.add(np.array([[2.0, 0.0, 0.0], [3.0, 0.0, 0.0]]), I4)
    assert e.value.code == capi.ERR_CAPACITY
    same_table(dev, ref)                                                              # as it was
    assert add_both(dev, ref, np.array([[2.0, 0.0, 0.0]]), I4)["rows"] == 3
    dev.close()


# ------------------------------------------------------------------ registration
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _T(res):
    return np.array(res.transformation[:]).reshape(4, 4)


def same_bits(a, b):
    assert np.array_equal(_bits(_T(a[0])), _bits(_T(b[0])))
    assert np.array_equal(_bits(a[1]), _bits(b[1]))
    assert (a[0].converged, a[0].num_iterations, a[0].history_len) == (b[0].converged, b[0].num_iterations, b[0].history_len)
    assert _bits(a[0].final_error) == _bits(b[0].final_error)


def test_register_is_align_on_the_table(ctx, oracle, drive16):
    frames, poses = drive16
    guess = synth.invert_transform(poses[0]) @ poses[1]
    guess[:3, 3] += (0.05, -0.03, 0.01)                                               # a start near the truth, not on it
    cfg = capi.Context.make_config(initial_transform=guess)
    scan = frames[1]
    dev = LocalMap(ctx, LocalMapConfig())
    dev.add(frames[0], I4)
    table, _keys = dev.points()
    d_scan = torch.from_numpy(np.ascontiguousarray(scan)).cuda()
    got = dev.register(scan, cfg)                                                     # the target the add prepared
    got_dev = dev.register_device(d_scan.data_ptr(), scan.shape[0], cfg)              # ... and prepared by the call
    got_rob = dev.register_robust(scan, cfg, HUBER)
    got_rob_dev = dev.register_robust_device(d_scan.data_ptr(), scan.shape[0], cfg, HUBER)
    dev.close()
    fresh = capi.Context(device=0)
    d_table = torch.from_numpy(table).cuda()
    same_bits(got, fresh.align(scan, table, cfg))
    same_bits(got_dev, fresh.align_device(d_scan.data_ptr(), scan.shape[0], d_table.data_ptr(), table.shape[0], cfg))
    want_rob = fresh.align_robust(scan, table, cfg, HUBER)
    for g in (got_rob, got_rob_dev):
        same_bits(g, want_rob)
        assert (g[2].weight_sum, g[2].pairs, g[2].rows) == (want_rob[2].weight_sum, want_rob[2].pairs, want_rob[2].rows)
    fresh.close()
    ref = oracle.icp_point_to_plane(scan, table, 50, 1e-6, 1e-9, initial_transform=guess, nthreads=4)
    for g in (got, got_dev):
        check_against(g[0], g[1], ref.transformation, ref.converged, ref.num_iterations, ref.error_history)
    ref = rr.robust_icp(scan, table, HUBER[0], HUBER[1], 0.0, 50, 1e-6, 1e-9, guess, orc=oracle)
    check_against(got_rob[0], got_rob[1], ref.transformation, ref.converged, ref.num_iterations, ref.error_history)


def test_remembered_target(drive16):
    """the add prepares the table as a target (its normals run during the add) and the next register finds it; after an
    unrelated align it is prepared again, and the result has the same bits"""
    frames, _poses = drive16
    ctx = capi.Context(device=0, profile=2)
    cfg = capi.Context.make_config()
    dev = LocalMap(ctx, LocalMapConfig())
    n0 = ctx.get_profile()["normals_launches"]
    dev.add(frames[0], I4)
    n1 = ctx.get_profile()["normals_launches"]
    first = dev.register(frames[1], cfg)
    n2 = ctx.get_profile()["normals_launches"]
    assert n1 > n0 and n2 == n1
    dev.clear()
    dev.add(frames[0], I4)
    n3 = ctx.get_profile()["normals_launches"]
    ctx.align(frames[3], frames[2], cfg)                                              # forgets the table
    n4 = ctx.get_profile()["normals_launches"]
    again = dev.register(frames[1], cfg)
    n5 = ctx.get_profile()["normals_launches"]
    assert n3 > n2 and n4 > n3 and n5 > n4
    same_bits(first, again)
    dev.close()
    ctx.close()


# ------------------------------------------------------------------ the drivers
def test_driver_in_lock_step(ctx, oracle, drive16):
    frames, poses = drive16
    config = LocalMapConfig()
    ref = lm.LocalMapRef(config.voxel_size, config.max_range, config.capacity)
    seen = []

    def on_frame(k, dev, r):
        if r is not None:                                                             # against the table BEFORE this add
            want = oracle.icp_point_to_plane(frames[k], ref.pts, 50, 1e-6, 1e-9, initial_transform=r.guess, nthreads=4)
            check_against(r, r.error_history, want.transformation, want.converged, want.num_iterations, want.error_history)
            pose = r.guess if ((not r.converged) or r.final_error > 1.0) else r.transformation
        else:
            pose = I4
        ref.add(frames[k], pose)                                                      # the GPU's own pose
        same_table(dev, ref)
        seen.append(k)

    track = odometry.run_odometry_local_map(frames, ctx, config, on_frame=on_frame)
    assert seen == list(range(12)) and track.map_rows[-1] == ref.size() and len(track.map_rows) == 12
    assert not any(track.gated)
    for k in range(1, 12):
        assert np.array_equal(track.deltas[k - 1], lm.invert(track.poses[k - 1]) @ track.poses[k])
    f2f = odometry.run_odometry(frames, odometry.gpu_align(ctx))
    ate, ate_f2f = odometry.absolute_trajectory_error(track, poses), odometry.absolute_trajectory_error(f2f, poses)
    print("16 x 600, 12 frames on the device: scan-to-map ATE %.4f m, frame-to-frame ATE %.4f m" % (ate, ate_f2f))
    assert ate < ate_f2f / 4.0


def test_run_slam_with_a_local_map(ctx, drive16):
    frames, _poses = drive16
    config = LocalMapConfig()
    track = odometry.run_odometry_local_map(frames, ctx, config)
    run = slam.run_slam(frames, ctx, odom_local_map=config)
    odom = [f for f in run.factors if f[0] == "odom"]
    assert len(odom) == 11
    for k, f in enumerate(odom):
        assert (f[1], f[2]) == (k, k + 1)
        assert np.array_equal(_bits(f[3]), _bits(track.deltas[k])) and f[4] == track.final_errors[k]
    run = slam.run_slam(frames, ctx, odom_local_map=config, odom_robust=HUBER)
    assert len(run.odom_weight_sums) == 11 and all(0.0 < w <= f.shape[0] for w, f in zip(run.odom_weight_sums, frames[1:]))
    with pytest.raises(ValueError):
        slam.run_slam(frames, ctx, odom_local_map=config, align=odometry.gpu_align(ctx))


# ------------------------------------------------------------------ error codes
def test_error_codes(ctx):
    L = capi.load_library()
    dp = C.POINTER(C.c_double)
    h = C.c_void_p()

    def make(**kw):
        c = capi.LocalMapConfig()
        L.icpmi_local_map_config_default(C.byref(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    c = make()
    assert (c.voxel_size, c.max_range, c.capacity) == (0.5, 100.0, 1 << 20)
    for bad in (dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(voxel_size=math.nan), dict(voxel_size=math.inf),
                dict(max_range=0.0), dict(max_range=-2.0), dict(max_range=math.nan), dict(max_range=math.inf),
                dict(capacity=0), dict(capacity=-5), dict(capacity=(1 << 27) + 1)):
        assert L.icpmi_local_map_create(ctx._h, C.byref(make(**bad)), C.byref(h)) == capi.ERR_ARG, bad
        assert not h.value
    small = make(capacity=64)
    assert L.icpmi_local_map_create(ctx._h, None, C.byref(h)) == capi.ERR_NULL
    assert L.icpmi_local_map_create(ctx._h, C.byref(small), None) == capi.ERR_NULL
    assert L.icpmi_local_map_create(None, C.byref(small), C.byref(h)) == capi.ERR_NULL
    assert L.icpmi_local_map_create(ctx._h, C.byref(small), C.byref(h)) == capi.OK and h.value
    xyz, pose = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]), np.eye(4).reshape(16).copy()
    info, n = capi.LocalMapInfo(), C.c_int64(-1)
    res, cfg, hist = capi.Result(), capi.Context.make_config(), np.zeros(51)
    rule, rinfo = capi.as_robust(HUBER), capi.RobustInfo()
    # an empty table
    assert L.icpmi_local_map_register(h, capi._dp(xyz), 2, C.byref(cfg), C.byref(res), capi._dp(hist), 51) == capi.ERR_EMPTY_TARGET
    assert L.icpmi_local_map_register_robust(h, capi._dp(xyz), 2, C.byref(cfg), C.byref(rule), C.byref(res), C.byref(rinfo),
                                             capi._dp(hist), 51) == capi.ERR_EMPTY_TARGET
    assert L.icpmi_local_map_size(h, C.byref(n)) == capi.OK and n.value == 0
    assert L.icpmi_local_map_points(h, None, None, 0, C.byref(n)) == capi.OK and n.value == 0
    # NULLs
    assert L.icpmi_local_map_add(None, capi._dp(xyz), 2, capi._dp(pose), C.byref(info)) == capi.ERR_NULL
    assert L.icpmi_local_map_add(h, None, 2, capi._dp(pose), C.byref(info)) == capi.ERR_NULL
    assert L.icpmi_local_map_add(h, capi._dp(xyz), 2, None, C.byref(info)) == capi.ERR_NULL
    assert L.icpmi_local_map_add_device(h, None, 2, capi._dp(pose), None) == capi.ERR_NULL
    assert L.icpmi_local_map_add_device(None, None, 0, capi._dp(pose), None) == capi.ERR_NULL
    assert L.icpmi_local_map_add_stream_frame(None, capi._dp(pose), None) == capi.ERR_NULL
    assert L.icpmi_local_map_add_stream_frame(h, None, None) == capi.ERR_NULL
    assert L.icpmi_local_map_size(None, C.byref(n)) == capi.ERR_NULL
    assert L.icpmi_local_map_size(h, None) == capi.ERR_NULL
    assert L.icpmi_local_map_points(None, None, None, 0, C.byref(n)) == capi.ERR_NULL
    assert L.icpmi_local_map_points(h, None, None, 0, None) == capi.ERR_NULL
    assert L.icpmi_local_map_clear(None) == capi.ERR_NULL
    # refused arguments; the table is untouched
    ctx.stream_reset()
    assert L.icpmi_local_map_add_stream_frame(h, capi._dp(pose), None) == capi.ERR_ARG        # no resident frame
    for bad in (math.nan, math.inf, -math.inf):
        p = pose.copy()
        p[7] = bad
        assert L.icpmi_local_map_add(h, capi._dp(xyz), 2, capi._dp(p), C.byref(info)) == capi.ERR_ARG
    assert L.icpmi_local_map_add(h, capi._dp(xyz), -1, capi._dp(pose), C.byref(info)) == capi.ERR_ARG
    assert L.icpmi_local_map_size(h, C.byref(n)) == capi.OK and n.value == 0
    # a table of two rows: info may be NULL, n == 0 with a NULL scan is legal
    assert L.icpmi_local_map_add(h, capi._dp(xyz), 2, capi._dp(pose), None) == capi.OK
    assert L.icpmi_local_map_add(h, None, 0, capi._dp(pose), C.byref(info)) == capi.OK and info.rows == 2
    assert L.icpmi_local_map_points(h, None, None, 0, C.byref(n)) == capi.OK and n.value == 2      # the size alone
    out, keys = np.zeros((2, 3)), np.zeros(2, dtype=np.uint64)
    assert L.icpmi_local_map_points(h, capi._dp(out), None, 1, C.byref(n)) == capi.ERR_CAPACITY
    assert L.icpmi_local_map_points(h, capi._dp(out), None, 2, C.byref(n)) == capi.OK and out.tolist() == xyz.tolist()
    assert L.icpmi_local_map_points(h, None, keys.ctypes.data_as(C.POINTER(C.c_uint64)), 2, C.byref(n)) == capi.OK
    assert keys[0] < keys[1]
    for args in ((None, 2, C.byref(cfg), C.byref(res), capi._dp(hist), 51), (capi._dp(xyz), 2, None, C.byref(res), capi._dp(hist), 51),
                 (capi._dp(xyz), 2, C.byref(cfg), None, capi._dp(hist), 51), (capi._dp(xyz), 2, C.byref(cfg), C.byref(res), None, 51)):
        assert L.icpmi_local_map_register(h, *args) == capi.ERR_NULL
    assert L.icpmi_local_map_register(None, capi._dp(xyz), 2, C.byref(cfg), C.byref(res), capi._dp(hist), 51) == capi.ERR_NULL
    assert L.icpmi_local_map_register_device(None, None, 2, C.byref(cfg), C.byref(res), capi._dp(hist), 51) == capi.ERR_NULL
    assert L.icpmi_local_map_register_device(h, None, 2, C.byref(cfg), C.byref(res), capi._dp(hist), 51) == capi.ERR_NULL
    assert L.icpmi_local_map_register(h, capi._dp(xyz), 2, C.byref(cfg), C.byref(res), capi._dp(hist), 3) == capi.ERR_CAPACITY
    assert L.icpmi_local_map_register_robust(h, capi._dp(xyz), 2, C.byref(cfg), None, C.byref(res), C.byref(rinfo),
                                             capi._dp(hist), 51) == capi.ERR_NULL
    assert L.icpmi_local_map_register_robust_device(h, None, 2, C.byref(cfg), None, C.byref(res), C.byref(rinfo),
                                                    capi._dp(hist), 51) == capi.ERR_NULL
    assert L.icpmi_local_map_register_robust_device(None, None, 2, C.byref(cfg), C.byref(rule), C.byref(res), C.byref(rinfo),
                                                    capi._dp(hist), 51) == capi.ERR_NULL
    assert L.icpmi_local_map_register(h, capi._dp(xyz), 0, C.byref(cfg), C.byref(res), capi._dp(hist), 51) == capi.ERR_EMPTY_SOURCE
    # clear, destroy
    assert L.icpmi_local_map_clear(h) == capi.OK
    assert L.icpmi_local_map_size(h, C.byref(n)) == capi.OK and n.value == 0
    assert L.icpmi_local_map_register(h, capi._dp(xyz), 2, C.byref(cfg), C.byref(res), capi._dp(hist), 51) == capi.ERR_EMPTY_TARGET
    assert L.icpmi_local_map_add(h, capi._dp(xyz), 2, capi._dp(pose), C.byref(info)) == capi.OK and info.inserted == 2
    L.icpmi_local_map_destroy(h)
    L.icpmi_local_map_destroy(None)
    del dp
