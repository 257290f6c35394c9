"""The device ray-cast (icpmi_map_raycast / icpmi_map_raster, csrc/raycast.h, GlobalMap.raycast) against its CPU
restatement (scripts/map_ref.py's MapRef.raycast, itself held to the definition by tests/test_raycast_reference.py):
the info fields and every byte of the raster, with no tolerance; the occupied cells against icpmi_map_finish's set."""
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
from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402
from lidar_slam_from_scratch_amd.global_map import GlobalMap  # noqa: E402
from test_gpu_map import _cells, _cloud, _device, _poses  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    """Fails loudly (no skip, no fallback) when the HIP library or the device is missing."""
    from lidar_slam_from_scratch_amd import build
    build.build_library()
    c = capi.Context(device=0)
    yield c
    c.close()


def _grid(**kw):
    return capi.Context.make_grid_config(**kw)


def _centred(poses):
    """the same track moved so that its middle pose sits at the origin: cells of both signs"""
    mid = poses[len(poses) // 2][:3, 3].copy()
    out = [p.copy() for p in poses]
    for p in out:
        p[:3, 3] -= mid
    return out


def _info(r):
    return (r.min_x, r.min_y, r.width, r.height, r.resolution, r.n_occupied, r.n_free)


def _assert_equal(got, want):
    assert _info(got) == _info(want)
    assert got.data.dtype == np.int8 and got.data.shape == want.data.shape == (want.height, want.width)
    assert np.array_equal(got.data, want.data)


def _store(ctx, sizes, seed=10):
    gm, ref = GlobalMap(ctx), map_ref.MapRef()
    for k, n in enumerate(sizes):
        c = _cloud(n, seed + k)
        if k % 2:
            d = _device(c)
            gm.add_frame_device(d.data_ptr() if n else 0, n)
            del d
        else:
            gm.add_frame(c)
        ref.add_frame(c)
    return gm, ref


def _R(grid):
    return int(np.ceil(grid.max_range / grid.resolution))


def test_raster_and_sets(ctx):
    sizes = [0, 1, 1500, 1023, 1025, 7, 20000]
    gm, ref = _store(ctx, sizes)
    poses = _centred(_poses(len(sizes), 2, step=3.0))
    grid = _grid()
    want = ref.raycast(poses, grid)
    # what the input must exercise, from the restatement's side
    g = map_ref.grid_kwargs(grid)
    carved, quadrants = set(), set()
    for cloud, T in zip(ref.clouds, poses):
        s = (int(np.floor(T[0, 3] / g["resolution"])), int(np.floor(T[1, 3] / g["resolution"])))
        hits = map_ref.hit_cells(map_ref.world_points(cloud, T), T[:2, 3], **g)
        carved.update(map(tuple, map_ref.bresenham_lockstep(s[0], s[1], hits[:, 0], hits[:, 1]).tolist()))
        if len(hits) > 100:
            quadrants.update(zip(np.sign(hits[:, 0] - s[0]).tolist(), np.sign(hits[:, 1] - s[1]).tolist()))
    assert carved & want.cells(map_ref.OCCUPIED)                          # a ray crosses another ray's hit cell
    assert {(1, 1), (1, -1), (-1, 1), (-1, -1)} <= quadrants
    assert want.n_free > want.n_occupied > 0 and want.min_x < 0 < want.min_x + want.width and want.min_y < 0
    cells, _ = gm.finish(poses, grid, 0.0)
    ctx.occupancy_clear()
    ctx.occupancy_update(np.array([[1e4, 1e4, 1.0]]), [1e4, 1e4 - 1.0, 0.0], grid)   # a sentinel cell in the context's set
    sentinel = ctx.occupancy_cells()
    assert len(sentinel) == 1
    got = gm.raycast(poses, grid)
    _assert_equal(got, want)
    y, x = np.nonzero(got.data == 100)
    assert set(zip((x + got.min_x).tolist(), (y + got.min_y).tolist())) == _cells(cells) and len(cells) == got.n_occupied
    assert np.array_equal(ctx.occupancy_cells(), sentinel)                # the context's set is not touched
    _assert_equal(gm.raycast(poses[:4], grid), ref.raycast(poses[:4], grid))   # fewer poses than frames
    _assert_equal(gm.raycast(poses + poses[:2]), ref.raycast(poses + poses[:2]))   # extra poses; the default grid
    gm.close()


def test_both_paths_same_answer(ctx):
    gm, ref = _store(ctx, [1500, 0, 1023, 1025, 7, 3000], seed=30)
    near = _cloud(400, 36) * [1.0 / 15.0, 1.0 / 15.0, 1.0]                # within 2 m of its sensor
    gm.add_frame(near)
    ref.add_frame(near)
    poses = _centred(_poses(7, 3, step=3.0))
    lds_max = capi.RAYCAST_LDS_MAX_R
    grids = [_grid(resolution=0.05, max_range=40.0),                      # R = 800: straight into the global plane
             _grid(resolution=0.2),                                       # R = 200: the window in LDS
             _grid(resolution=1.0),
             _grid(resolution=0.25, max_range=0.25 * lds_max),            # the largest window LDS takes, and the next
             _grid(resolution=0.25, max_range=0.25 * (lds_max + 1)),
             _grid(resolution=0.25, max_range=0.25 * 351),                # the largest window within 64 KiB, and the
             _grid(resolution=0.25, max_range=0.25 * 352)]                # next: LDS the launch has to ask for
    assert [_R(g) for g in grids] == [800, 200, 40, lds_max, lds_max + 1, 351, 352] and 352 <= lds_max < 800
    for grid in grids:
        want = ref.raycast(poses, grid)
        assert want.n_free > 0 and want.n_occupied > 0
        _assert_equal(gm.raycast(poses, grid), want)
    # at 1 m cells some hits lie in their sensor's own cell
    g = map_ref.grid_kwargs(grids[2])
    own = 0
    for cloud, T in zip(ref.clouds, poses):
        hits = map_ref.hit_cells(map_ref.world_points(cloud, T), T[:2, 3], **g)
        own += int(np.count_nonzero((hits[:, 0] == np.floor(T[0, 3])) & (hits[:, 1] == np.floor(T[1, 3]))))
    assert own > 0
    gm.close()


def test_tile_and_window_edges(ctx):
    grid = _grid()                                                        # max_range 40 at 0.2 m: R = 200
    R, mr = _R(grid), grid.max_range
    t = np.array([0.25, -0.75, 0.0])                                      # exact in binary: dx, dy below are exact
    d = 28.28427                                                          # sqrt(2 d^2) < 40
    edge = [(mr, 0), (-mr, 0), (0, mr), (0, -mr),                         # r == max_range exactly, on the axes ...
            (24, 32), (-24, 32), (24, -32), (-24, -32), (32, 24), (-32, -24),   # ... and off them (3-4-5)
            (d, d), (-d, d), (d, -d), (-d, -d),                           # the diagonals
            (0.5, 0), (-0.5, 0), (0, 0.5), (0.3, 0.41), (-0.3, -0.41)]    # r == 0.5, and just above
    out = [(mr + 1e-9, 0), (0, -mr - 1e-9), (0.4999999, 0), (0, -0.4999999)]    # these cast no ray
    rows = np.array([[x, y, 1.0] for x, y in edge + out])
    T = synth.make_transform([0.0, 0.0, 0.0], t)
    ring = np.random.default_rng(5).uniform(0.0, 2 * np.pi, size=(1025,))
    full = np.stack([30.0 * np.cos(ring), 30.0 * np.sin(ring), np.full_like(ring, 1.0)], axis=1)   # every row a hit
    gm, ref = GlobalMap(ctx), map_ref.MapRef()
    for c in (rows, full[:1024], full):
        gm.add_frame(c)
        ref.add_frame(c)
    g = map_ref.grid_kwargs(grid)
    hits = map_ref.hit_cells(map_ref.world_points(rows, T), t[:2], **g)
    assert len(hits) == len(edge)
    s = np.floor(t[:2] / grid.resolution).astype(np.int64)
    off = hits - s
    assert np.abs(off).max() == R and {(R, 0), (-R, 0), (0, R), (0, -R)} <= set(map(tuple, off.tolist()))   # the farthest a hit lies
    for c in (full[:1024], full):
        assert len(map_ref.hit_cells(map_ref.world_points(c, T), t[:2], **g)) == len(c)
    want = ref.raycast([T], grid)
    assert (want.min_x, want.width) == (s[0] - R - 5, 2 * R + 11) and (want.min_y, want.height) == (s[1] - R - 5, 2 * R + 11)
    _assert_equal(gm.raycast([T], grid), want)
    _assert_equal(gm.raycast([T] * 3, grid), ref.raycast([T] * 3, grid))
    gm.close()


def test_errors_and_repeatability(ctx):
    L = capi.load_library()
    gm, ref = _store(ctx, [300, 0, 2500], seed=40)
    poses = _poses(3, 4)
    P = np.ascontiguousarray(np.stack(poses))
    dp = capi._dp(P)
    grid = _grid()
    info = capi.RasterInfo()

    def raster():
        """(info fields, bytes) through the C calls"""
        i = capi.RasterInfo()
        assert L.icpmi_map_raster(gm._h, None, 0, C.byref(i)) == capi.OK
        data = np.full(i.width * i.height, 7, dtype=np.int8)
        assert L.icpmi_map_raster(gm._h, data.ctypes.data_as(C.POINTER(C.c_int8)), data.size, None) == capi.OK
        return (i.min_x, i.min_y, i.width, i.height, i.resolution, i.n_occupied, i.n_free), data

    assert raster()[0] == (0, 0, 0, 0, 0.0, 0, 0)                         # before any raycast: all zeros
    assert L.icpmi_map_raycast(gm._h, None, 3, C.byref(grid), C.byref(info)) == capi.ERR_NULL
    assert L.icpmi_map_raycast(gm._h, dp, 3, None, C.byref(info)) == capi.ERR_NULL
    assert raster()[0] == (0, 0, 0, 0, 0.0, 0, 0)
    assert L.icpmi_map_raycast(gm._h, dp, 3, C.byref(grid), C.byref(info)) == capi.OK
    want = ref.raycast(poses, grid)
    first = raster()
    assert first[0] == _info(want) == (info.min_x, info.min_y, info.width, info.height, info.resolution, info.n_occupied, info.n_free)
    assert np.array_equal(first[1].reshape(want.height, want.width), want.data)
    bad = P.copy()
    bad[2, 1, 1] = np.nan
    far = P.copy()
    far[2, :2, 3] += 1e5                                                  # 10^5 m apart on both axes: 2.5e11 cells
    huge = P.copy()
    huge[0, 0, 3] = 0.2 * 2.0**31                                         # a sensor cell past 2^31 - 2 - R - 6
    fails = [(bad, grid), (far, grid), (huge, grid), (P, _grid(resolution=0.0)), (P, _grid(resolution=-0.2)),
             (P, _grid(resolution=float("nan"))), (P, _grid(resolution=float("inf"))),
             (P, _grid(resolution=0.005, max_range=20.5)),                # R = 4100 > 4096
             (P, _grid(max_range=float("inf")))]
    for poses_bad, g in fails:
        marker = capi.RasterInfo(width=-3)
        assert L.icpmi_map_raycast(gm._h, capi._dp(poses_bad), 3, C.byref(g), C.byref(marker)) == capi.ERR_ARG
        assert marker.width == -3                                         # info is not written by a failed call
        again = raster()
        assert again[0] == first[0] and np.array_equal(again[1], first[1])    # the previous raster, byte for byte
    assert _R(_grid(resolution=0.005, max_range=20.48)) == capi.RAYCAST_MAX_R
    small = np.empty(want.width * want.height - 1, dtype=np.int8)
    assert L.icpmi_map_raster(gm._h, small.ctypes.data_as(C.POINTER(C.c_int8)), small.size, C.byref(info)) == capi.ERR_CAPACITY
    assert info.width == want.width
    with pytest.raises(capi.IcpError) as e:
        gm.raycast(bad, grid)
    assert e.value.code == capi.ERR_ARG
    a, b = gm.raycast(poses, grid), gm.raycast(poses, grid)               # twice: identical bytes
    _assert_equal(a, b)
    _assert_equal(a, want)
    # an all-filtered store and an empty one: 0 x 0, and that is then the handle's raster
    gm.add_frame(_cloud(50, 1))
    z = gm.raycast(poses[:2], _grid(height_min=50.0, height_max=60.0))
    assert _info(z) == (0, 0, 0, 0, 0.2, 0, 0) and z.data.shape == (0, 0)
    assert raster()[0] == (0, 0, 0, 0, 0.2, 0, 0)
    empty = GlobalMap(ctx)
    for r in (empty.raycast(poses, grid), empty.raycast([], grid), gm.raycast([], grid)):
        assert _info(r) == (0, 0, 0, 0, 0.2, 0, 0) and r.data.shape == (0, 0)
    empty.close()
    gm.close()


def test_run_slam_with_raycast(ctx):
    """test_run_slam_with_global_map's drive: the device's raster equals the restatement's, and asking for it changes
    nothing else."""
    from lidar_slam_from_scratch_amd import slam
    order = list(range(60)) + list(range(59, -1, -1))
    cache = {f: synth.lidar_frame(f, beams=32, azimuths=900, **synth.DRIVE_200) for f in set(order)}
    frames = [cache[f] for f in order]
    gm, gm2 = GlobalMap(ctx), GlobalMap(ctx)
    run = slam.run_slam(frames, ctx, global_map=gm, raycast=True)
    ref = slam.run_slam(frames, ctx, global_map=map_ref.MapRef(), raycast=True)
    plain = slam.run_slam(frames, ctx, global_map=gm2)
    assert plain.raster is None and run.closures
    _assert_equal(run.raster, ref.raster)
    assert run.raster.n_free > run.raster.n_occupied > 0
    assert len(run.poses) == len(plain.poses) and all(np.array_equal(a, b) for a, b in zip(run.poses, plain.poses))
    assert len(run.factors) == len(plain.factors)
    for f, g in zip(run.factors, plain.factors):
        assert len(f) == len(g)
        assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(f, g))
    assert [(c.match_frame, c.query_frame) for c in run.closures] == [(c.match_frame, c.query_frame) for c in plain.closures]
    assert np.array_equal(run.cells, plain.cells) and len(run.cells) == run.raster.n_occupied
    assert np.array_equal(run.published_map.view(np.uint64), plain.published_map.view(np.uint64))
    gm.close()
    gm2.close()


def test_two_million_rows(ctx):
    """About 2 M rows (a few synthetic scans reused along a drive): many frames' windows overlap in the plane."""
    base = [synth.lidar_frame(f) for f in range(0, 40, 10)]
    per = np.mean([b.shape[0] for b in base])
    F = int(np.ceil(2.0e6 / per))
    gm, ref = GlobalMap(ctx), map_ref.MapRef()
    for k in range(F):
        gm.add_frame(base[k % len(base)])
        ref.add_frame(base[k % len(base)])
    assert gm.size()[1] >= 2_000_000
    poses = _poses(F, 5, step=1.2)
    want = ref.raycast(poses)
    assert want.n_free > want.n_occupied > 0
    _assert_equal(gm.raycast(poses), want)
    gm.close()
