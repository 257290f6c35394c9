"""The static map on the device (icpmi_map_world_static / icpmi_map_finish_static / icpmi_map_static_labels,
csrc/static_map.h, GlobalMap.world_static) against its CPU restatement (scripts/static_map_ref.py, itself held to the
contract by tests/test_static_map_reference.py): the labels of every used frame, the kept world rows, the published map
and every info field, byte for byte and with no tolerance; the ties to icpmi_map_world, icpmi_map_finish and the live
counts; and that a refused call changes nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import torch  # noqa: F401  (first: one HIP runtime per process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import map_ref  # noqa: E402
import static_map_ref as ref  # noqa: E402
from lidar_slam_from_scratch_amd import capi, ground, synth  # noqa: E402
from lidar_slam_from_scratch_amd.global_map import GlobalMap  # noqa: E402
from test_gpu_counts import _assert_equal, _centred, _grid  # noqa: E402
from test_gpu_map import _poses, _row_set, _same  # noqa: E402

pytestmark = pytest.mark.gpu

U8P = C.POINTER(C.c_uint8)
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500]


@pytest.fixture()
def ctx():
    """Fails loudly (no skip, no fallback) when the HIP library or the device is missing."""
    from lidar_slam_from_scratch_amd import build
    build.build_library()
    c = capi.Context(device=0)
    yield c
    c.close()


def _square(n, seed, half=24.0):
    """n rows in a square three max_range wide (the grid below: max_range 16), most of them in the band"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-half, half, size=(n, 3))
    c[:, 2] = rng.uniform(-0.2, 2.5, size=n)
    return c


def _edge_grid():
    g = _grid(resolution=1.0, max_range=16.0)
    assert int(np.ceil(g.max_range / g.resolution)) == 16
    return g


def _fill(ctx, clouds):
    gm = GlobalMap(ctx)
    for c in clouds:
        gm.add_frame(c)
    return gm


def _info(i):
    return ref.StaticInfo(i.rows, i.voting, i.dropped, i.kept)


def _labels(gm, used):
    return [gm.static_labels(k) for k in range(used)]


def _assert_static(gm, clouds, poses, grid, rule, firsts=(0,), ground_labels=None, voxel=1.0):
    """world_static for every `first`, static_labels of every used frame and finish_static against the restatement"""
    used = min(len(clouds), len(poses))
    want_all, want_labels, want_info = ref.world_static(clouds, poses, grid, rule, 0, ground_labels)
    for first in firsts:
        want = ref.world_static(clouds, poses, grid, rule, first, ground_labels)[0] if first else want_all
        got, info = gm.world_static(poses, grid, rule, first)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), first
        assert _info(info) == want_info, first
        got_labels = _labels(gm, used)                                    # all used frames, whatever first is
        assert all(a.dtype == np.uint8 and a.tobytes() == b.tobytes() for a, b in zip(got_labels, want_labels)), first
    with pytest.raises(capi.IcpError) as e:
        gm.static_labels(used)                                            # a frame the call did not use
    assert e.value.code == capi.ERR_ARG
    published, info = gm.finish_static(poses, grid, rule, voxel)
    want_pub = map_ref.orc.voxel_downsample(want_all, voxel) if len(want_all) else np.zeros((0, 3))
    assert np.array_equal(_row_set(published), _row_set(want_pub)) and _info(info) == want_info
    assert all(a.tobytes() == b.tobytes() for a, b in zip(_labels(gm, used), want_labels))
    return want_all, want_labels, want_info


# ------------------------------------------------------------------------------------------------------ dispatch edges

@pytest.fixture(scope="module")
def edges():
    clouds = [_square(n, 300 + k) for k, n in enumerate(SIZES)]
    poses = _centred(_poses(len(SIZES), 5, step=3.0))                     # a few cells apart
    return clouds, poses


def test_dispatch_edges(ctx, edges):
    clouds, poses = edges
    grid, rule = _edge_grid(), (50, 2)
    gm = _fill(ctx, clouds)
    used = len(SIZES)
    world, labels, info = _assert_static(gm, clouds, poses, grid, rule, firsts=(0, 6, 11, used, used + 7))
    # what the input must exercise, from the restatement's side
    counts = ref.counts_of(clouds, poses, grid)[0]
    assert counts.max_hits > 2 and counts.max_misses > 2 and int(np.count_nonzero((counts.hits > 0) & (counts.misses > 0))) > 100
    assert info.rows == sum(SIZES) and 0 < info.dropped < info.voting < info.rows
    assert all((lab == 2).any() and (lab != 2).any() for lab in labels[5:])          # every larger frame compacts
    assert len(ref.world_static(clouds, poses, grid, rule, used)[0]) == 0
    recent = gm.recent_clouds_static(poses, grid, rule, 4)                # one cloud per frame, the dropped rows gone
    assert len(recent) == 4
    for k, r in zip(range(8, 12), recent):
        assert r.tobytes() == map_ref.world_points(clouds[k], poses[k])[labels[k] != 2].tobytes()
    # fewer poses than frames: the used frames alone
    _assert_static(gm, clouds, poses[:9], grid, rule, firsts=(0, 4))
    # the count alone, a short cap, and the next good call
    L, P = gm._lib, np.ascontiguousarray(np.stack(poses))
    r, n, si = capi.StaticRule(*rule), C.c_int64(-1), capi.StaticInfo()
    assert L.icpmi_map_world_static(gm._h, capi._dp(P), used, C.byref(grid), C.byref(r), 0, None, 0, C.byref(n), C.byref(si)) == capi.OK
    assert n.value == len(world) == info.kept and _info(si) == info
    small = np.full((n.value - 1, 3), 7.0)
    assert L.icpmi_map_world_static(gm._h, capi._dp(P), used, C.byref(grid), C.byref(r), 0, capi._dp(small), n.value - 1, C.byref(n),
                                    None) == capi.ERR_CAPACITY
    assert (small == 7.0).all()
    got, _ = gm.world_static(poses, grid, rule)
    assert got.tobytes() == world.tobytes()
    out = np.empty((1, 3))
    nm = C.c_int64(-1)
    assert L.icpmi_map_finish_static(gm._h, capi._dp(P), used, C.byref(grid), C.byref(r), 1.0, capi._dp(out), 1, C.byref(nm),
                                     None) == capi.ERR_CAPACITY
    assert L.icpmi_map_finish_static(gm._h, capi._dp(P), used, C.byref(grid), C.byref(r), 0.0, capi._dp(out), 1, C.byref(nm),
                                     C.byref(si)) == capi.OK and nm.value == 0 and _info(si) == info      # no filter asked for
    _assert_static(gm, clouds, poses, grid, rule)
    gm.close()


def test_keep_patterns(ctx):
    """rows of a cell every other frame looks through (dropped) and of a cell nothing looks through (kept), laid out so
    that the first, or the last, kept row of a tile falls in each of its four waves; a frame that is dropped whole and
    one that is kept whole"""
    T = synth.make_transform(np.array([0.0, 0.0, 0.3]), np.array([0.3, 0.2, 0.0]))      # sensor cell (0, 0)
    Tinv = synth.invert_transform(T)
    rng = np.random.default_rng(77)

    def rows(pattern):
        """pattern: bool per row, True = a row of the solid cell (0, 5), False = of the ghost cell (4, 0)"""
        world = np.where(np.asarray(pattern)[:, None], [0.5, 5.5, 1.0], [4.5, 0.5, 1.0]) + rng.uniform(-0.2, 0.2, size=(len(pattern), 3))
        return synth.apply_transform(Tinv, world)

    patterns = []
    for w in range(4):
        first = np.zeros(1100, dtype=bool)
        first[64 * w + 5:] = True                                         # the tile's first kept row in wave w of sweep 0
        last = np.ones(1100, dtype=bool)
        last[768 + 64 * w + 8:1024] = False                               # ... its last kept row in wave w of sweep 3
        patterns += [first, last]
    patterns.append(np.zeros(300, dtype=bool))                            # dropped whole
    patterns.append(np.ones(300, dtype=bool))                             # kept whole
    patterns.append(rng.integers(0, 2, size=2500).astype(bool))
    clouds = [rows(p) for p in patterns]
    carver = synth.apply_transform(Tinv, np.array([[8.5, 0.5, 1.0]]))     # a hit behind the ghost cell, on its line
    clouds += [carver] * 12                                               # more frames look through it than hit it
    poses = [T] * len(clouds)
    grid, rule = _edge_grid(), (50, 3)
    gm = _fill(ctx, clouds)
    _, labels, info = _assert_static(gm, clouds, poses, grid, rule, firsts=(0, 3, 8, 9))
    for p, lab in zip(patterns, labels):                                  # the restatement sees the patterns as laid out
        assert np.array_equal(lab, np.where(p, 1, 2))
    assert all((lab == 1).all() for lab in labels[len(patterns):])
    assert info.dropped == sum(int((~p).sum()) for p in patterns) and info.voting == info.rows
    gm.close()


# ---------------------------------------------------------------------------------------- the ties to the existing path

def test_min_probability_zero_is_the_old_path(ctx, edges):
    clouds, poses = edges
    grid = _edge_grid()
    gm = _fill(ctx, clouds)
    for first in (0, 6, len(SIZES)):
        got, info = gm.world_static(poses, grid, (0, 1), first)
        assert got.tobytes() == gm.world(poses, first).tobytes()
        assert info.dropped == 0 and info.kept == info.rows == sum(SIZES)
    labels = np.concatenate(_labels(gm, len(SIZES)))
    assert set(np.unique(labels).tolist()) == {0, 1} and int((labels == 1).sum()) == info.voting
    published, _ = gm.finish_static(poses, grid, (0, 1), 1.0)
    assert published.tobytes() == gm.finish(poses, grid, 1.0)[1].tobytes()
    recent, plain = gm.recent_clouds_static(poses, grid, (0, 1), 5), gm.recent_clouds(poses, 5)
    assert len(recent) == len(plain) == 5 and all(a.tobytes() == b.tobytes() for a, b in zip(recent, plain))
    gm.close()


def test_live_interplay(ctx, edges):
    clouds, poses = edges
    grid, rule = _edge_grid(), (50, 2)
    gm = _fill(ctx, clouds[:8])
    got, info = gm.world_static(poses[:8], grid, rule)
    assert (info.live.frames_cast, info.live.rebuilt) == (8, 0)
    assert got.tobytes() == ref.world_static(clouds[:8], poses[:8], grid, rule)[0].tobytes()
    live = gm.live_counts()[0]
    _assert_equal(live, gm.raycast_counts(poses[:8], grid))               # the live counts are the batch call's
    assert bytes(gm.live_counts()[1]) == bytes(info.live)
    for c in clouds[8:]:
        gm.add_frame(c)
    got, info = gm.world_static(poses, grid, rule)                        # four more frames: only they are cast
    assert (info.live.frames_cast, info.live.rebuilt) == (4, 0)
    want = ref.world_static(clouds, poses, grid, rule)
    assert got.tobytes() == want[0].tobytes() and _info(info) == want[2]
    i = gm.live_update(poses, grid)                                       # a plain update in between: nothing to do
    assert (i.frames_cast, i.rebuilt) == (0, 0)
    published, info = gm.finish_static(poses, grid, rule, 1.0)
    assert (info.live.frames_cast, info.live.rebuilt) == (0, 0) and _info(info) == want[2]
    assert np.array_equal(_row_set(published), _row_set(map_ref.orc.voxel_downsample(want[0], 1.0)))
    _assert_equal(gm.live_counts()[0], gm.raycast_counts(poses, grid))
    moved = [p.copy() for p in poses]
    moved[3][0, 3] += 1.0                                                 # an optimize moved a pose: a rebuild
    got, info = gm.world_static(moved, grid, rule)
    assert (info.live.frames_cast, info.live.rebuilt) == (len(SIZES), 1)
    want = ref.world_static(clouds, moved, grid, rule)
    assert got.tobytes() == want[0].tobytes() and _info(info) == want[2]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(_labels(gm, len(SIZES)), want[1]))
    _assert_equal(gm.live_counts()[0], gm.raycast_counts(moved, grid))
    gm.close()


# -------------------------------------------------------------------------------------------------- ground, and the drive

def test_with_ground(ctx):
    frames, poses = [], []
    for f in range(4):
        pts, _, T = synth.ramp_frame(10 * f, 41, beams=16, azimuths=600)
        frames.append(pts)
        poses.append(T)
    gm = _fill(ctx, frames)
    gm.set_ground(ground.GroundConfig())
    gl = [gm.ground_labels(k) for k in range(4)]
    grid = _grid(resolution=0.5, max_range=30.0)
    _, labels, info = _assert_static(gm, frames, poses, grid, (50, 2), firsts=(0, 2), ground_labels=gl)
    for lab, g in zip(labels, gl):
        assert not lab[g != capi.GROUND_OBSTACLE].any()                   # ground and ignored rows: label 0
    assert info.voting > 1000 and info.dropped > 0
    gm.set_ground(None)                                                   # the band again: a rebuild, other labels
    got, i2 = gm.world_static(poses, grid, (50, 2))
    want = ref.world_static(frames, poses, grid, (50, 2))
    assert got.tobytes() == want[0].tobytes() and _info(i2) == want[2] and i2.live.rebuilt == 1
    gm.close()


def test_moving_car_drive(ctx):
    """byte parity on the drive whose effect tests/test_static_map_reference.py asserts on the CPU"""
    clouds, poses, grid, _, _ = ref.moving_car_drive()
    g = _grid(**grid)
    gm = _fill(ctx, clouds)
    _, _, info = _assert_static(gm, clouds, poses, g, None, firsts=(0,), voxel=0.5)
    assert 70000 < info.rows < 90000 and info.dropped > 1000
    gm.close()


# ------------------------------------------------------------------------------------------------------- refused calls

def _state(gm, ctx, used):
    lc, li = gm.live_counts()
    c, r = gm.counts(), gm.raster()
    return (b"".join(lab.tobytes() for lab in _labels(gm, used)), bytes(li), lc.hits.tobytes(), lc.misses.tobytes(),
            lc.probability.tobytes(), c.hits.tobytes(), c.misses.tobytes(), c.probability.tobytes(), r.data.tobytes(),
            ctx.occupancy_cells().tobytes())


def test_refused_arguments_change_nothing(ctx, edges):
    clouds, poses = edges
    clouds, poses = clouds[4:10], poses[4:10]
    grid = _edge_grid()
    gm = _fill(ctx, clouds)
    L = gm._lib
    P = np.ascontiguousarray(np.stack(poses))
    dp, n, nm, si = capi._dp(P), C.c_int64(-1), C.c_int64(-1), capi.StaticInfo()
    good = capi.StaticRule(50, 2)
    lab = np.zeros(4096, dtype=np.uint8)
    # before any call: no labels
    assert L.icpmi_map_static_labels(gm._h, 0, lab.ctypes.data_as(U8P), 4096, C.byref(n)) == capi.ERR_ARG
    gm.finish(poses, grid, 1.0), gm.raycast(poses, grid), gm.raycast_counts(poses, grid)        # the batch products
    want, _ = gm.world_static(poses, grid, good)
    before = _state(gm, ctx, 6)
    out = np.full((len(want) + 1, 3), 7.0)

    def world(h=gm._h, p=dp, k=6, g=C.byref(grid), r=C.byref(good), first=0, n_out=C.byref(n)):
        return L.icpmi_map_world_static(h, p, k, g, r, first, capi._dp(out), len(out), n_out, C.byref(si))

    def finish(h=gm._h, p=dp, k=6, g=C.byref(grid), r=C.byref(good)):
        return L.icpmi_map_finish_static(h, p, k, g, r, 1.0, capi._dp(out), len(out), C.byref(nm), C.byref(si))

    for call in (world, finish):
        assert call(h=None) == capi.ERR_NULL and call(p=None) == capi.ERR_NULL
        assert call(g=None) == capi.ERR_NULL and call(r=None) == capi.ERR_NULL
        for bad in (capi.StaticRule(-1, 2), capi.StaticRule(101, 2), capi.StaticRule(50, 0), capi.StaticRule(50, -3),
                    capi.StaticRule(50, 2, 1)):
            assert call(r=C.byref(bad)) == capi.ERR_ARG
        nan = P.copy()
        nan[2, 1, 3] = np.nan
        assert call(p=capi._dp(nan)) == capi.ERR_ARG                      # a non-finite used pose
        assert call(k=-1) == capi.ERR_ARG
        assert call(g=C.byref(_grid(resolution=0.0))) == capi.ERR_ARG and call(g=C.byref(_grid(resolution=1e-3, max_range=16.0))) == capi.ERR_ARG
    assert world(first=-1) == capi.ERR_ARG and world(n_out=None) == capi.ERR_NULL
    assert (out == 7.0).all() and n.value == -1 and nm.value == -1 and bytes(si) == bytes(capi.StaticInfo())
    assert L.icpmi_map_static_labels(None, 0, lab.ctypes.data_as(U8P), 4096, C.byref(n)) == capi.ERR_NULL
    assert L.icpmi_map_static_labels(gm._h, 0, lab.ctypes.data_as(U8P), 4096, None) == capi.ERR_NULL
    assert L.icpmi_map_static_labels(gm._h, 6, lab.ctypes.data_as(U8P), 4096, C.byref(n)) == capi.ERR_ARG      # not a used frame
    assert L.icpmi_map_static_labels(gm._h, -1, lab.ctypes.data_as(U8P), 4096, C.byref(n)) == capi.ERR_ARG
    assert L.icpmi_map_static_labels(gm._h, 5, lab.ctypes.data_as(U8P), 10, C.byref(n)) == capi.ERR_CAPACITY and n.value == len(clouds[5])
    assert L.icpmi_map_static_labels(gm._h, 5, None, 0, C.byref(n)) == capi.OK and n.value == len(clouds[5])
    assert _state(gm, ctx, 6) == before
    assert world() == capi.OK and n.value == len(want) and out[:len(want)].tobytes() == want.tobytes()
    assert (si.live.frames_cast, si.live.rebuilt) == (0, 0)                # the live state stood: nothing to cast
    after = _state(gm, ctx, 6)                                            # (the live info now says frames_cast 0)
    assert after[0] == before[0] and after[2:] == before[2:]
    gm.close()


# ----------------------------------------------------------------------------------------------------------- run_slam

def test_run_slam_static_map(ctx):
    from lidar_slam_from_scratch_amd import slam
    frames = [synth.lidar_frame(f, beams=32, azimuths=600) for f in range(6)]
    grid = _grid(height_min=-1.4, height_max=0.5)
    gm, plain_map = GlobalMap(ctx), GlobalMap(ctx)
    run = slam.run_slam(frames, ctx, global_map=gm, grid=grid, static_map=(50, 3))
    plain = slam.run_slam(frames, ctx, global_map=plain_map, grid=grid)
    direct, info = gm.finish_static(run.poses, grid, (50, 3), 1.0)
    assert run.published_map_static.tobytes() == direct.tobytes() and len(direct) > 0
    assert bytes(run.static_info)[:32] == bytes(info)[:32] and run.static_info.rows == sum(len(f) for f in frames)
    want, want_info = ref.finish_static(frames, run.poses, grid, (50, 3), 1.0)
    assert np.array_equal(_row_set(direct), _row_set(want)) and _info(info) == want_info
    # without it: what run_slam returned before
    assert plain.published_map_static is None and plain.static_info is None
    assert _same(run.published_map, plain.published_map) and np.array_equal(run.cells, plain.cells)
    assert all(np.array_equal(a, b) for a, b in zip(run.poses, plain.poses)) and len(run.poses) == len(plain.poses)
    nomap = slam.run_slam(frames, ctx, static_map=(50, 3))                # ignored without a global map
    assert nomap.published_map_static is None and len(nomap.poses) == len(plain.poses)
    gm.close(), plain_map.close()
