"""The device's hit / miss counts (icpmi_map_raycast_counts / icpmi_map_counts, csrc/raycount.h,
GlobalMap.raycast_counts) against their CPU restatement (scripts/map_ref.py's MapRef.raycast_counts, itself held to
the definition by tests/test_counts_reference.py): the info fields and every byte of the three arrays, with no
tolerance; and the three relations to the device's own free / occupied / unknown raster."""
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
from test_gpu_map import _cloud, _device, _poses  # noqa: E402

pytestmark = pytest.mark.gpu

U16P, I8P = C.POINTER(C.c_uint16), C.POINTER(C.c_int8)


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


def _info(c):
    return (c.min_x, c.min_y, c.width, c.height, c.resolution, c.n_observed, c.n_hit_cells, c.max_hits, c.max_misses,
            c.frames_used)


def _assert_equal(got, want):
    assert _info(got) == _info(want)
    for a, b, dt in ((got.hits, want.hits, np.uint16), (got.misses, want.misses, np.uint16),
                     (got.probability, want.probability, np.int8)):
        assert a.dtype == b.dtype == dt and a.shape == b.shape == (want.height, want.width)
        assert np.array_equal(a, b)


def _assert_relations(c, r):
    """hits > 0 <=> the raster is 100; hits == 0 and misses > 0 <=> it is 0; otherwise both are -1; an equal box"""
    assert (c.min_x, c.min_y, c.width, c.height, c.resolution) == (r.min_x, r.min_y, r.width, r.height, r.resolution)
    assert np.array_equal(c.hits > 0, r.data == 100)
    assert np.array_equal((c.hits == 0) & (c.misses > 0), r.data == 0)
    assert np.array_equal(c.probability == -1, r.data == -1)
    assert c.n_hit_cells == r.n_occupied and c.n_observed == r.n_occupied + r.n_free


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


def test_counts_and_relations(ctx):
    sizes = [0, 1, 1500, 1023, 1025, 7, 20000]
    gm, ref = _store(ctx, sizes)
    poses = _centred(_poses(len(sizes), 2, step=3.0))
    grid = _grid()
    want = ref.raycast_counts(poses, grid)
    # what the input must exercise, from the restatement's side
    assert want.n_hit_cells == 9495 and int(np.count_nonzero(want.misses)) == 82686
    assert int(np.count_nonzero((want.hits > 0) & (want.misses > 0))) == 5367
    assert (want.max_hits, want.max_misses, want.frames_used) == (3, 5, 7)
    assert set(np.unique(want.probability).tolist()) == {-1, 0, 20, 25, 33, 50, 67, 100}
    assert want.min_x < 0 < want.min_x + want.width and want.min_y < 0
    ctx.occupancy_clear()
    ctx.occupancy_update(np.array([[1e4, 1e4, 1.0]]), [1e4, 1e4 - 1.0, 0.0], grid)   # a sentinel cell in the context's set
    sentinel = ctx.occupancy_cells()
    assert len(sentinel) == 1
    got = gm.raycast_counts(poses, grid)
    _assert_equal(got, want)
    _assert_relations(got, gm.raycast(poses, grid))
    assert np.array_equal(ctx.occupancy_cells(), sentinel)                # the context's set is not touched
    few = gm.raycast_counts(poses[:4], grid)                              # fewer poses than frames
    _assert_equal(few, ref.raycast_counts(poses[:4], grid))
    _assert_relations(few, gm.raycast(poses[:4], grid))
    assert few.frames_used == 4
    _assert_equal(gm.raycast_counts(poses + poses[:2]), want)             # extra poses; the default grid
    gm.close()


def test_both_window_homes(ctx):
    gm, ref = _store(ctx, [1500, 0, 1023, 1025, 7, 3000], seed=30)
    near = _cloud(400, 36) * [1.0 / 15.0, 1.0 / 15.0, 1.0]                # within 2 m of its sensor
    gm.add_frame(near)
    ref.add_frame(near)
    poses = _centred(_poses(7, 3, step=3.0))
    lds_max = capi.RAYCOUNT_LDS_MAX_R
    grids = [_grid(resolution=0.05, max_range=40.0),                      # R = 800: the windows in device scratch
             _grid(resolution=0.2),                                       # R = 200: the windows in LDS
             _grid(resolution=1.0),
             _grid(resolution=0.25, max_range=0.25 * lds_max),            # the largest pair LDS takes, and the next
             _grid(resolution=0.25, max_range=0.25 * (lds_max + 1)),
             _grid(resolution=0.25, max_range=0.25 * 239),                # the largest pair within 64 KiB, and the
             _grid(resolution=0.25, max_range=0.25 * 240)]                # next: LDS the launch has to ask for
    assert [_R(g) for g in grids] == [800, 200, 40, 392, 393, 239, 240] and lds_max == 392
    for grid in grids:
        want = ref.raycast_counts(poses, grid)
        assert want.max_hits > 1 and want.max_misses > 1 and want.n_observed > want.n_hit_cells > 0
        _assert_equal(gm.raycast_counts(poses, grid), want)
    gm.close()


def test_range_and_stride_edges(ctx):
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
    want = ref.raycast_counts([T], grid)
    assert (want.min_x, want.width) == (s[0] - R - 5, 2 * R + 11) and (want.min_y, want.height) == (s[1] - R - 5, 2 * R + 11)
    assert (want.max_hits, want.max_misses, want.frames_used) == (1, 1, 1)
    _assert_equal(gm.raycast_counts([T], grid), want)
    want3 = ref.raycast_counts([T] * 3, grid)
    assert want3.max_hits == 2 and want3.max_misses == 3                  # the two ring frames share their hit cells
    _assert_equal(gm.raycast_counts([T] * 3, grid), want3)
    gm.close()


def test_dedup_rounding_tie_and_frame_cap(ctx):
    L = capi.load_library()
    T = synth.make_transform([0.0, 0.0, 0.0], [0.05, 0.05, 0.0])
    gm, ref = GlobalMap(ctx), map_ref.MapRef()
    frames = [np.tile([[10.05, 0.05, 1.0]], (1500, 1))] + [np.array([[20.05, 0.05, 1.0]])] * 7
    for c in frames:
        gm.add_frame(c)
        ref.add_frame(c)
    got = gm.raycast_counts([T] * 8)
    at = lambda x, y: (int(got.hits[y - got.min_y, x - got.min_x]), int(got.misses[y - got.min_y, x - got.min_x]),  # noqa: E731
                       int(got.probability[y - got.min_y, x - got.min_x]))
    assert at(50, 0) == (1, 7, 13)                                        # 1,500 rows add 1; 12.5 rounds half up
    assert at(100, 0) == (7, 0, 100) and at(0, 0) == (0, 8, 0)
    assert int(np.count_nonzero(got.misses)) == 100
    _assert_equal(got, ref.raycast_counts([T] * 8))
    gm.close()
    # 65,536 one-row frames on one pose: 65,535 of them are counted, one more is refused
    cap = capi.RAYCOUNT_MAX_FRAMES
    assert cap == 65535
    row = np.array([[20.05, 0.05, 1.0]])
    big = GlobalMap(ctx)
    for _ in range(cap + 1):
        assert L.icpmi_map_add_frame(big._h, capi._dp(row), 1) == capi.OK
    assert big.size() == (cap + 1, cap + 1)
    one = map_ref.MapRef()
    one.add_frame(row)
    w1 = one.raycast_counts([T])
    assert (w1.n_observed, w1.n_hit_cells, w1.max_hits, w1.max_misses) == (101, 1, 1, 1)
    P = np.ascontiguousarray(np.tile(T, (cap + 1, 1, 1)))
    got = big.raycast_counts(P[:cap])
    assert _info(got) == _info(w1)[:7] + (cap, cap, cap)
    assert np.array_equal(got.hits, w1.hits * np.uint16(cap)) and np.array_equal(got.misses, w1.misses * np.uint16(cap))
    assert np.array_equal(got.probability, w1.probability) and got.hits.max() == got.misses.max() == 65535
    marker = capi.CountsInfo(width=-3)
    grid = _grid()
    assert L.icpmi_map_raycast_counts(big._h, capi._dp(P), cap + 1, C.byref(grid), C.byref(marker)) == capi.ERR_ARG
    assert marker.width == -3
    _assert_equal(big.counts(), got)                                      # the previous result
    big.close()


def test_errors_and_repeatability(ctx):
    L = capi.load_library()
    gm, ref = _store(ctx, [300, 0, 2500], seed=40)
    poses = _poses(3, 4)
    P = np.ascontiguousarray(np.stack(poses))
    dp = capi._dp(P)
    grid = _grid()
    info = capi.CountsInfo()
    fields = [f for f, _ in capi.CountsInfo._fields_]

    def counts():
        """(info fields, the three arrays) through the C calls"""
        i = capi.CountsInfo()
        assert L.icpmi_map_counts(gm._h, None, None, None, 0, C.byref(i)) == capi.OK
        n = i.width * i.height
        h, m, p = np.full(n, 7, dtype=np.uint16), np.full(n, 7, dtype=np.uint16), np.full(n, 7, dtype=np.int8)
        assert L.icpmi_map_counts(gm._h, h.ctypes.data_as(U16P), m.ctypes.data_as(U16P), p.ctypes.data_as(I8P), n, None) == capi.OK
        return tuple(getattr(i, f) for f in fields), h, m, p

    def same(a, b):
        return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))

    zeros = (0, 0, 0, 0, 0.0, 0, 0, 0, 0, 0, 0)
    assert counts()[0] == zeros                                           # before any call: all zeros
    assert L.icpmi_map_raycast_counts(gm._h, None, 3, C.byref(grid), C.byref(info)) == capi.ERR_NULL
    assert L.icpmi_map_raycast_counts(gm._h, dp, 3, None, C.byref(info)) == capi.ERR_NULL
    assert L.icpmi_map_raycast_counts(None, dp, 3, C.byref(grid), C.byref(info)) == capi.ERR_NULL
    assert L.icpmi_map_counts(None, None, None, None, 0, C.byref(info)) == capi.ERR_NULL
    assert counts()[0] == zeros
    assert L.icpmi_map_raycast_counts(gm._h, dp, 3, C.byref(grid), C.byref(info)) == capi.OK
    want = ref.raycast_counts(poses, grid)
    first = counts()
    assert first[0][:10] == _info(want) == tuple(getattr(info, f) for f in fields[:10])
    shape = (want.height, want.width)
    assert np.array_equal(first[1].reshape(shape), want.hits) and np.array_equal(first[2].reshape(shape), want.misses)
    assert np.array_equal(first[3].reshape(shape), want.probability)
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
        marker = capi.CountsInfo(width=-3)
        assert L.icpmi_map_raycast_counts(gm._h, capi._dp(poses_bad), 3, C.byref(g), C.byref(marker)) == capi.ERR_ARG
        assert marker.width == -3                                         # info is not written by a failed call
        assert same(counts(), first)                                      # the previous counts, byte for byte
    assert L.icpmi_map_raycast_counts(gm._h, dp, -1, C.byref(grid), None) == capi.ERR_ARG
    # any of the three arrays may be NULL; too little room for one that is given is refused
    n = want.width * want.height
    only = np.full(n, 7, dtype=np.int8)
    assert L.icpmi_map_counts(gm._h, None, None, only.ctypes.data_as(I8P), n, None) == capi.OK
    assert np.array_equal(only, first[3])
    only = np.full(n, 7, dtype=np.uint16)
    assert L.icpmi_map_counts(gm._h, None, only.ctypes.data_as(U16P), None, n, None) == capi.OK
    assert np.array_equal(only, first[2])
    assert L.icpmi_map_counts(gm._h, only.ctypes.data_as(U16P), None, None, n, None) == capi.OK
    assert np.array_equal(only, first[1])
    only[:] = 7
    assert L.icpmi_map_counts(gm._h, only.ctypes.data_as(U16P), None, None, n - 1, C.byref(info)) == capi.ERR_CAPACITY
    assert info.width == want.width and (only == 7).all()
    assert L.icpmi_map_counts(gm._h, None, None, only.view(np.int8).ctypes.data_as(I8P), n - 1, None) == capi.ERR_CAPACITY
    assert L.icpmi_map_counts(gm._h, None, None, None, 0, None) == capi.OK
    with pytest.raises(capi.IcpError) as e:
        gm.raycast_counts(bad, grid)
    assert e.value.code == capi.ERR_ARG
    a, b = gm.raycast_counts(poses, grid), gm.raycast_counts(poses, grid)    # twice: identical bytes
    _assert_equal(a, b)
    _assert_equal(a, want)
    # the two products are independent: each call leaves the other's result alone
    assert gm.raster().data.shape == (0, 0)                               # no raycast yet, whatever raycast_counts did
    r2 = gm.raycast(poses[:1], grid)
    _assert_equal(gm.counts(), want)
    c1 = gm.raycast_counts(poses, _grid(resolution=0.5))
    r_now = gm.raster()
    assert (r_now.min_x, r_now.width, r_now.resolution) == (r2.min_x, r2.width, 0.2) and np.array_equal(r_now.data, r2.data)
    gm.raycast(poses, grid)
    _assert_equal(gm.counts(), c1)
    # an all-filtered store and an empty one: 0 x 0, and that is then the handle's result
    gm.add_frame(_cloud(50, 1))
    z = gm.raycast_counts(poses[:2], _grid(height_min=50.0, height_max=60.0))
    assert _info(z) == (0, 0, 0, 0, 0.2, 0, 0, 0, 0, 2) and z.hits.shape == z.misses.shape == z.probability.shape == (0, 0)
    assert counts()[0] == (0, 0, 0, 0, 0.2, 0, 0, 0, 0, 2, 0)
    empty = GlobalMap(ctx)
    for c, used in ((empty.raycast_counts(poses, grid), 0), (empty.raycast_counts([], grid), 0), (gm.raycast_counts([], grid), 0)):
        assert _info(c) == (0, 0, 0, 0, 0.2, 0, 0, 0, 0, used) and c.hits.shape == (0, 0)
    empty.close()
    gm.close()


def test_run_slam_with_counts(ctx):
    """test_run_slam_with_raycast's out-and-back drive: the run's counts equal the restatement on the run's poses, and
    asking for them changes nothing else."""
    from lidar_slam_from_scratch_amd import slam
    order = list(range(60)) + list(range(59, -1, -1))
    cache = {f: synth.lidar_frame(f, beams=32, azimuths=900, **synth.DRIVE_200) for f in set(order)}
    frames = [cache[f] for f in order]
    gm, gm2 = GlobalMap(ctx), GlobalMap(ctx)
    run = slam.run_slam(frames, ctx, global_map=gm, counts=True)
    plain = slam.run_slam(frames, ctx, global_map=gm2)
    assert plain.counts is None and run.raster is None and run.closures
    ref = map_ref.MapRef()
    for f in frames:
        ref.add_frame(f)
    want = ref.raycast_counts(run.poses)
    _assert_equal(run.counts, want)
    assert want.max_hits > 2 and want.max_misses > 2 and 0 < want.n_hit_cells < want.n_observed
    assert len(set(np.unique(want.probability).tolist())) > 3             # a spread of values, not the three states
    assert len(run.poses) == len(plain.poses) and all(np.array_equal(a, b) for a, b in zip(run.poses, plain.poses))
    assert len(run.factors) == len(plain.factors)
    for f, g in zip(run.factors, plain.factors):
        assert len(f) == len(g)
        assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(f, g))
    assert [(c.match_frame, c.query_frame) for c in run.closures] == [(c.match_frame, c.query_frame) for c in plain.closures]
    assert np.array_equal(run.cells, plain.cells) and len(run.cells) == run.counts.n_hit_cells
    assert np.array_equal(run.published_map.view(np.uint64), plain.published_map.view(np.uint64))
    gm.close()
    gm2.close()


def test_two_million_rows(ctx):
    """About 2 M rows (a few synthetic scans reused along a drive): many frames' windows overlap in the plane.

    The restatement gives, for these 233 frames 1.2 m apart: 1,477,370 observed cells, 69,867 of them hit, max hits 4
    (the four scans are taken at different places, so a moved copy seldom lands a return in another copy's cell) and max
    misses 27 (rays of many frames cross the same ground).  The spread is asserted loosely before the exact comparison."""
    base = [synth.lidar_frame(f) for f in range(0, 40, 10)]
    per = np.mean([b.shape[0] for b in base])
    F = int(np.ceil(2.0e6 / per))
    gm, ref = GlobalMap(ctx), map_ref.MapRef()
    for k in range(F):
        gm.add_frame(base[k % len(base)])
        ref.add_frame(base[k % len(base)])
    assert gm.size()[1] >= 2_000_000
    poses = _poses(F, 5, step=1.2)
    want = ref.raycast_counts(poses)
    assert want.max_hits > 1 and want.max_misses > 10 and want.n_observed > want.n_hit_cells > 0
    _assert_equal(gm.raycast_counts(poses), want)
    gm.close()
