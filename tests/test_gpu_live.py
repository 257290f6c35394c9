"""The counts kept while the node drives (icpmi_map_live_update / icpmi_map_live_counts / icpmi_map_live_clear,
csrc/live_counts.h, GlobalMap.live_update) against the CPU restatement of the batch call they must equal
(scripts/map_ref.py's MapRef.raycast_counts): every info field and every byte of the three arrays after every update,
with no tolerance; what each update reports it cast; and that the plane only grows."""
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
from test_gpu_counts import _assert_equal, _centred, _grid, _info, _R, _store  # noqa: E402
from test_gpu_map import _cloud, _poses  # noqa: E402

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


def _box(i):
    return (i.plane_x0, i.plane_y0, i.plane_w, i.plane_h)


def _holds(outer, inner):
    return (outer[0] <= inner[0] and outer[1] <= inner[1] and outer[0] + outer[2] >= inner[0] + inner[2]
            and outer[1] + outer[3] >= inner[1] + inner[3])


def _update(gm, poses, grid, want, frames_cast, rebuilt):
    """one live_update: what it reports, and the live counts against `want`"""
    info = gm.live_update(poses, grid)
    assert (info.frames_cast, info.rebuilt) == (frames_cast, rebuilt)
    got, again = gm.live_counts()
    assert bytes(again) == bytes(info)                                    # live_counts reports the update's info
    assert _info(got) == tuple(getattr(info.counts, f) for f in ("min_x", "min_y", "width", "height", "resolution", "n_observed",
                                                                 "n_hit_cells", "max_hits", "max_misses", "frames_used"))
    _assert_equal(got, want)
    if want.width:                                                        # the plane holds every observed cell
        assert _holds(_box(info), (want.min_x + 5, want.min_y + 5, want.width - 10, want.height - 10))
    return info


def test_step_by_step(ctx):
    G, rows = capi.LIVE_CARVE_GROUPS, capi.LIVE_CARVE_ROWS
    assert (G, rows) == (16, 1024)
    # a workgroup's share of a frame's rows is ceil(rows / min(G, ceil(rows / 1024))): 1, 2 and G workgroups, full
    # and short last shares, and fewer rows than workgroups
    sizes = [0, 1, 7, 1500, 1023, 1025, 5, G * rows - 1, G * rows, G * rows + 1, 20000]
    gm, ref = GlobalMap(ctx), map_ref.MapRef()
    poses = _centred(_poses(len(sizes), 2, step=3.0))
    grid = _grid()
    assert _R(grid) == 200
    boxes = []
    for k, n in enumerate(sizes):
        c = _cloud(n, 10 + k)
        gm.add_frame(c)
        ref.add_frame(c)
        want = ref.raycast_counts(poses[:k + 1], grid)
        info = _update(gm, poses[:k + 1], grid, want, 1, 0)
        boxes.append(_box(info))
        assert k == 0 or _holds(boxes[k], boxes[k - 1])
    # what the input must exercise, from the restatement's side
    assert want.max_hits > 1 and want.max_misses > 1 and int(np.count_nonzero((want.hits > 0) & (want.misses > 0))) > 1000
    assert want.min_x < 0 < want.min_x + want.width and want.min_y < 0 < want.min_y + want.height
    assert want.frames_used == len(sizes)
    _assert_equal(gm.raycast_counts(poses, grid), want)                   # the device's own batch call
    _assert_equal(gm.live_counts()[0], want)                              # ... which left the live counts alone
    gm.close()


def test_several_pending_frames(ctx):
    sizes = [1500, 0, 1023, 1025, 7, 3000, 2100, 900, 1, 2500, 1800, 40]
    clouds = [_cloud(n, 60 + k) for k, n in enumerate(sizes)]
    poses = _centred(_poses(len(sizes), 7, step=3.0))
    grid = _grid()
    ref = map_ref.MapRef()
    for c in clouds:
        ref.add_frame(c)
    want = ref.raycast_counts(poses, grid)
    assert want.max_hits > 1 and want.max_misses > 2
    gm = GlobalMap(ctx)
    for c in clouds[:3]:
        gm.add_frame(c)
    _update(gm, poses[:3], grid, ref.raycast_counts(poses[:3], grid), 3, 0)        # three frames, one update
    for c in clouds[3:]:
        gm.add_frame(c)
    a = _update(gm, poses, grid, want, 9, 0)                                       # nine more: past the per-frame pair
    fresh = GlobalMap(ctx)
    for c in clouds:
        fresh.add_frame(c)
    b = _update(fresh, poses, grid, want, len(sizes), 0)                           # all at once into a fresh handle
    assert bytes(a.counts) == bytes(b.counts)
    for x, y in zip(gm.live_counts()[0].__dict__.values(), fresh.live_counts()[0].__dict__.values()):
        assert np.array_equal(x, y)
    gm.close()
    fresh.close()


def test_growth(ctx):
    """a track that leaves the plane on +x, -y, -x and +y in turn, 15 m (75 cells) a step: the box grows by half its
    extent on the side crossed, so the first steps of every leg move the plane"""
    legs = [(1, 0)] * 9 + [(0, -1)] * 8 + [(-1, 0)] * 10 + [(0, 1)] * 13
    at = np.array([-32.0, 41.0])
    track = [at.copy()]
    for d in legs:
        at = at + 15.0 * np.array(d)
        track.append(at.copy())
    assert len(track) == 41
    poses = [synth.make_transform([0.0, 0.0, 0.05 * k], [x, y, 0.0]) for k, (x, y) in enumerate(track)]
    xs, ys = [p[0] for p in track], [p[1] for p in track]
    assert min(xs) < 0 < max(xs) and min(ys) < 0 < max(ys)
    gm, ref = GlobalMap(ctx), map_ref.MapRef()
    grid = _grid()
    moved, boxes, sides = 0, [], set()
    for k in range(len(poses)):
        c = _cloud(500, 400 + k)
        gm.add_frame(c)
        ref.add_frame(c)
        if k % 8 == 7 or k == len(poses) - 1:
            info = _update(gm, poses[:k + 1], grid, ref.raycast_counts(poses[:k + 1], grid), 1, 0)
        else:
            info = gm.live_update(poses[:k + 1], grid)
            assert (info.frames_cast, info.rebuilt) == (1, 0)
        box = _box(info)
        s = np.floor(np.array(track[k]) / grid.resolution).astype(int)
        assert _holds(box, (s[0] - 201, s[1] - 201, 403, 403))            # the frame's window
        if boxes:
            old = boxes[-1]
            assert _holds(box, old) and info.moved == int(box != old)     # it only ever grows
            sides |= {n for n, grew in (("-x", box[0] < old[0]), ("-y", box[1] < old[1]),
                                        ("+x", box[0] + box[2] > old[0] + old[2]), ("+y", box[1] + box[3] > old[1] + old[3])) if grew}
        else:
            assert info.moved == 0 and box == (s[0] - 201, s[1] - 201, 403, 403)
        moved += info.moved
        boxes.append(box)
    assert moved >= 3 and sides == {"+x", "-y", "-x", "+y"}
    assert boxes[-1][0] < 0 < boxes[-1][0] + boxes[-1][2] and boxes[-1][1] < 0 < boxes[-1][1] + boxes[-1][3]
    gm.close()


def test_rebuild_triggers(ctx):
    sizes = [1500, 0, 1023, 2500, 7, 3000]
    gm, ref = _store(ctx, sizes, seed=70)
    poses = _centred(_poses(len(sizes), 8, step=3.0))
    grid = _grid()
    want = ref.raycast_counts(poses, grid)
    _update(gm, poses, grid, want, 6, 0)                                  # the first update: everything, nothing discarded
    first = gm.live_counts()[0]
    i2 = _update(gm, poses, grid, want, 0, 0)                             # the same call twice: nothing cast
    assert i2.moved == 0
    _assert_equal(gm.live_counts()[0], first)
    _update(gm, poses + poses[:1], grid, want, 0, 0)                      # an extra pose without a frame: nothing new
    moved = [p.copy() for p in poses]
    moved[3][1, 3] = np.nextafter(moved[3][1, 3], np.inf)                 # one bit of one pose already cast
    assert int(np.sum(np.stack(moved).view(np.uint64) != np.stack(poses).view(np.uint64))) == 1
    _update(gm, moved, grid, ref.raycast_counts(moved, grid), 6, 1)
    _update(gm, moved[:4], grid, ref.raycast_counts(moved[:4], grid), 4, 1)          # fewer poses than were cast
    _update(gm, moved, grid, ref.raycast_counts(moved, grid), 2, 0)                  # and the rest again, incrementally
    other = _grid(resolution=0.5)
    _update(gm, moved, other, ref.raycast_counts(moved, other), 6, 1)               # another grid
    same_values = _grid(resolution=0.5)
    _update(gm, moved, same_values, ref.raycast_counts(moved, other), 0, 0)          # an equal grid in another object
    gm.live_clear()
    z, zi = gm.live_counts()
    assert _info(z) == (0, 0, 0, 0, 0.0, 0, 0, 0, 0, 0) and bytes(zi) == bytes(capi.LiveInfo())
    _update(gm, moved, other, ref.raycast_counts(moved, other), 6, 0)               # after a clear: all again, not "rebuilt"
    e = _update(gm, [], other, ref.raycast_counts([], other), 0, 1)                  # no poses: the counts are dropped
    assert _box(e) == (0, 0, 0, 0)
    gm.close()


def test_window_homes(ctx):
    clouds = [_cloud(n, 30 + k) for k, n in enumerate([1500, 0, 1023, 1025, 7, 3000])]
    clouds.append(_cloud(400, 36) * [1.0 / 15.0, 1.0 / 15.0, 1.0])       # within 2 m of its sensor
    poses = _centred(_poses(7, 3, step=3.0))
    lds_max = capi.RAYCOUNT_LDS_MAX_R
    grids = [_grid(resolution=0.05, max_range=40.0), _grid(resolution=0.2), _grid(resolution=1.0),
             _grid(resolution=0.25, max_range=0.25 * lds_max), _grid(resolution=0.25, max_range=0.25 * (lds_max + 1)),
             _grid(resolution=0.25, max_range=0.25 * 239), _grid(resolution=0.25, max_range=0.25 * 240)]
    assert [_R(g) for g in grids] == [800, 200, 40, 392, 393, 239, 240] and lds_max == 392
    for grid in grids:
        gm, ref = GlobalMap(ctx), map_ref.MapRef()
        for k, c in enumerate(clouds):
            gm.add_frame(c)
            ref.add_frame(c)
            want = ref.raycast_counts(poses[:k + 1], grid)
            _update(gm, poses[:k + 1], grid, want, 1, 0)
        assert want.max_hits > 1 and want.max_misses > 1 and want.n_observed > want.n_hit_cells > 0
        gm.close()


def test_range_edges(ctx):
    grid = _grid()                                                        # max_range 40 at 0.2 m: R = 200
    R, mr = _R(grid), grid.max_range
    t = np.array([0.25, -0.75, 0.0])
    d = 28.28427
    edge = [(mr, 0), (-mr, 0), (0, mr), (0, -mr), (24, 32), (-24, 32), (24, -32), (-24, -32), (32, 24), (-32, -24),
            (d, d), (-d, d), (d, -d), (-d, -d), (0.5, 0), (-0.5, 0), (0, 0.5), (0.3, 0.41), (-0.3, -0.41)]
    out = [(mr + 1e-9, 0), (0, -mr - 1e-9), (0.4999999, 0), (0, -0.4999999)]    # these cast no ray
    rows = np.array([[x, y, 1.0] for x, y in edge + out])
    T = synth.make_transform([0.0, 0.0, 0.0], t)
    ring = np.random.default_rng(5).uniform(0.0, 2 * np.pi, size=(1025,))
    full = np.stack([30.0 * np.cos(ring), 30.0 * np.sin(ring), np.full_like(ring, 1.0)], axis=1)
    gm, ref = GlobalMap(ctx), map_ref.MapRef()
    s = np.floor(t[:2] / grid.resolution).astype(np.int64)
    for k, c in enumerate((rows, full[:1024], full)):
        gm.add_frame(c)
        ref.add_frame(c)
        want = ref.raycast_counts([T] * (k + 1), grid)
        info = _update(gm, [T] * (k + 1), grid, want, 1, 0)
        if k == 0:                                                        # hits at exactly R cells on the axes
            assert (want.min_x, want.width) == (s[0] - R - 5, 2 * R + 11) and (want.min_y, want.height) == (s[1] - R - 5, 2 * R + 11)
            assert (info.counts.width, info.counts.height) == (2 * R + 11, 2 * R + 11)
        assert _box(info) == (s[0] - R - 1, s[1] - R - 1, 2 * R + 3, 2 * R + 3) and info.moved == 0
    assert want.max_hits == 2 and want.max_misses == 3
    gm.close()


def test_errors_and_independence(ctx):
    L = capi.load_library()
    gm, ref = _store(ctx, [300, 0, 2500], seed=40)
    poses = _poses(3, 4)
    P = np.ascontiguousarray(np.stack(poses))
    dp = capi._dp(P)
    grid = _grid()

    def live():
        """(the info's bytes, the three arrays) through the C calls"""
        i = capi.LiveInfo()
        assert L.icpmi_map_live_counts(gm._h, None, None, None, 0, C.byref(i)) == capi.OK
        n = i.counts.width * i.counts.height
        h, m, p = np.full(n, 7, dtype=np.uint16), np.full(n, 7, dtype=np.uint16), np.full(n, 7, dtype=np.int8)
        assert L.icpmi_map_live_counts(gm._h, h.ctypes.data_as(U16P), m.ctypes.data_as(U16P), p.ctypes.data_as(I8P), n, None) == capi.OK
        return bytes(i), h, m, p

    def same(a, b):
        return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))

    zero = bytes(capi.LiveInfo())
    assert live()[0] == zero and live()[1].size == 0                      # before any update: all zeros, 0 x 0
    info = capi.LiveInfo()
    assert L.icpmi_map_live_update(gm._h, None, 3, C.byref(grid), C.byref(info)) == capi.ERR_NULL
    assert L.icpmi_map_live_update(gm._h, dp, 3, None, C.byref(info)) == capi.ERR_NULL
    assert L.icpmi_map_live_update(None, dp, 3, C.byref(grid), C.byref(info)) == capi.ERR_NULL
    assert L.icpmi_map_live_counts(None, None, None, None, 0, C.byref(info)) == capi.ERR_NULL
    assert L.icpmi_map_live_clear(None) == capi.ERR_NULL
    assert bytes(info) == zero and live()[0] == zero
    # the context's set, the batch counts and the raster before any live call
    ctx.occupancy_clear()
    ctx.occupancy_update(np.array([[1e4, 1e4, 1.0]]), [1e4, 1e4 - 1.0, 0.0], grid)
    sentinel = ctx.occupancy_cells()
    batch = gm.raycast_counts(poses[:1], _grid(resolution=0.5))
    raster = gm.raycast(poses[:1], _grid(resolution=0.5))
    assert L.icpmi_map_live_update(gm._h, dp, 2, C.byref(grid), C.byref(info)) == capi.OK
    assert (info.frames_cast, info.rebuilt) == (2, 0)
    first = live()
    assert first[0] == bytes(info)
    want2 = ref.raycast_counts(poses[:2], grid)
    _assert_equal(gm.live_counts()[0], want2)
    bad = P.copy()
    bad[2, 1, 1] = np.nan
    far = P.copy()
    far[2, :2, 3] += 1e5                                                  # 10^5 m apart on both axes: 2.5e11 cells
    huge = P.copy()
    huge[2, 0, 3] = 0.2 * 2.0**31                                         # a sensor cell past 2^31 - 2 - R - 6
    early = P.copy()
    early[0, 0, 3] = 0.2 * 2.0**31                                        # ... in a frame cast already: a rebuild, refused
    fails = [(bad, grid), (far, grid), (huge, grid), (early, grid), (P, _grid(resolution=0.0)), (P, _grid(resolution=-0.2)),
             (P, _grid(resolution=float("nan"))), (P, _grid(resolution=float("inf"))),
             (P, _grid(resolution=0.005, max_range=20.5)),                # R = 4100 > 4096
             (P, _grid(max_range=float("inf")))]
    for poses_bad, g in fails:
        marker = capi.LiveInfo(frames_cast=-3)
        assert L.icpmi_map_live_update(gm._h, capi._dp(poses_bad), 3, C.byref(g), C.byref(marker)) == capi.ERR_ARG
        assert marker.frames_cast == -3 and bytes(marker.counts) == bytes(capi.CountsInfo())   # info is not written
        assert same(live(), first)                                        # the live counts, byte for byte
    assert L.icpmi_map_live_update(gm._h, dp, -1, C.byref(grid), None) == capi.ERR_ARG
    assert same(live(), first)
    with pytest.raises(capi.IcpError) as e:
        gm.live_update(bad, grid)
    assert e.value.code == capi.ERR_ARG
    # the next good update is still incremental
    want = ref.raycast_counts(poses, grid)
    _update(gm, poses, grid, want, 1, 0)
    # any of the three arrays may be NULL; too little room for one that is given is refused
    full = live()
    n = want.width * want.height
    only = np.full(n, 7, dtype=np.int8)
    assert L.icpmi_map_live_counts(gm._h, None, None, only.ctypes.data_as(I8P), n, None) == capi.OK
    assert np.array_equal(only, full[3]) and np.array_equal(only.reshape(want.height, want.width), want.probability)
    only = np.full(n, 7, dtype=np.uint16)
    assert L.icpmi_map_live_counts(gm._h, None, only.ctypes.data_as(U16P), None, n, None) == capi.OK
    assert np.array_equal(only, full[2])
    only[:] = 7
    assert L.icpmi_map_live_counts(gm._h, only.ctypes.data_as(U16P), None, None, n - 1, C.byref(info)) == capi.ERR_CAPACITY
    assert info.counts.width == want.width and (only == 7).all()
    # independence: the live calls left the other products alone, and the other calls leave the live counts alone
    assert np.array_equal(ctx.occupancy_cells(), sentinel)
    _assert_equal(gm.counts(), batch)
    r_now = gm.raster()
    assert (r_now.min_x, r_now.width, r_now.resolution) == (raster.min_x, raster.width, 0.5) and np.array_equal(r_now.data, raster.data)
    gm.raycast_counts(poses, _grid(resolution=1.0))
    gm.raycast(poses, _grid(resolution=1.0))
    gm.finish(poses, grid)
    assert same(live(), full)
    gm.add_frame(_cloud(800, 44))
    more = poses + _poses(4, 4)[3:]
    ref.add_frame(_cloud(800, 44))
    _update(gm, more, grid, ref.raycast_counts(more, grid), 1, 0)         # ... and it goes on incrementally
    # an all-filtered store and an empty one: 0 x 0 and no plane
    none = _grid(height_min=50.0, height_max=60.0)
    z = _update(gm, more, none, ref.raycast_counts(more, none), 4, 1)
    assert (z.counts.width, z.counts.height, z.counts.frames_used) == (0, 0, 4) and z.plane_w > 0
    empty = GlobalMap(ctx)
    for p in (poses, []):
        i = empty.live_update(p, grid)
        assert (i.frames_cast, i.rebuilt, i.moved, i.counts.frames_used) == (0, 0, 0, 0) and _box(i) == (0, 0, 0, 0)
        assert empty.live_counts()[0].hits.shape == (0, 0)
    empty.close()
    gm.close()


def test_frame_cap(ctx):
    """65,536 one-row frames on one pose: 65,535 of them are cast by one update (the batch kernels: more pending
    frames than the per-frame pair takes), and one more pose is refused"""
    L = capi.load_library()
    T = synth.make_transform([0.0, 0.0, 0.0], [0.05, 0.05, 0.0])
    cap = capi.RAYCOUNT_MAX_FRAMES
    row = np.array([[20.05, 0.05, 1.0]])
    big = GlobalMap(ctx)
    for _ in range(cap + 1):
        assert L.icpmi_map_add_frame(big._h, capi._dp(row), 1) == capi.OK
    one = map_ref.MapRef()
    one.add_frame(row)
    w1 = one.raycast_counts([T])
    assert (w1.n_observed, w1.n_hit_cells, w1.max_hits, w1.max_misses) == (101, 1, 1, 1)
    P = np.ascontiguousarray(np.tile(T, (cap + 1, 1, 1)))
    info = big.live_update(P[:cap])
    assert (info.frames_cast, info.rebuilt) == (cap, 0)
    got = big.live_counts()[0]
    assert _info(got) == _info(w1)[:7] + (cap, cap, cap)
    assert np.array_equal(got.hits, w1.hits * np.uint16(cap)) and np.array_equal(got.misses, w1.misses * np.uint16(cap))
    assert np.array_equal(got.probability, w1.probability) and got.hits.max() == got.misses.max() == 65535
    marker = capi.LiveInfo(frames_cast=-3)
    grid = _grid()
    assert L.icpmi_map_live_update(big._h, capi._dp(P), cap + 1, C.byref(grid), C.byref(marker)) == capi.ERR_ARG
    assert marker.frames_cast == -3
    after = big.live_counts()[0]
    _assert_equal(after, got)
    big.close()


def test_run_slam_live(ctx):
    """test_run_slam_with_counts' out-and-back drive with live=True: the live counts equal the restatement on the
    run's poses and the run's own batch counts; the log shows one frame a step and a rebuild after each optimize that
    moved the poses; and asking for them changes nothing else."""
    from lidar_slam_from_scratch_amd import slam
    order = list(range(60)) + list(range(59, -1, -1))
    cache = {f: synth.lidar_frame(f, beams=32, azimuths=900, **synth.DRIVE_200) for f in set(order)}
    frames = [cache[f] for f in order]
    gm, gm2 = GlobalMap(ctx), GlobalMap(ctx)
    run = slam.run_slam(frames, ctx, global_map=gm, counts=True, live=True)
    plain = slam.run_slam(frames, ctx, global_map=gm2)
    assert plain.live is None and plain.live_log == [] and run.closures
    ref = map_ref.MapRef()
    for f in frames:
        ref.add_frame(f)
    want = ref.raycast_counts(run.poses)
    _assert_equal(run.live, want)
    _assert_equal(run.live, run.counts)
    assert want.max_hits > 2 and want.max_misses > 2 and 0 < want.n_hit_cells < want.n_observed
    # the log: one update per frame, one per optimize, and the last one before live_counts
    oks = [ok for _, ok, _ in run.optimizations]
    assert len(run.live_log) == len(frames) + len(oks) + 1 and any(oks)
    log = iter(run.live_log)
    assert next(log) == (1, 0)                                            # the first frame
    opt = iter(run.optimizations)
    for k in range(1, len(frames)):
        assert next(log) == (1, 0), k                                     # one frame a step, closures or not
        if k % 10 == 0 and k > 50 and any(c.query_frame == k for c in run.closures):
            tag, ok, _ = next(opt)
            assert tag == k
            assert next(log) == ((k + 1, 1) if ok else (0, 0)), k         # the poses moved: everything again
    tag, ok, _ = next(opt)
    # (the last optimize adds no closure: it may leave every pose as it was, bit for bit, and then nothing is cast)
    assert tag == "end" and next(log) in (((len(frames), 1), (0, 0)) if ok else ((0, 0),))
    assert sum(r for _, r in run.live_log) >= 1
    assert next(log) == (0, 0) and next(log, None) is None
    assert len(run.poses) == len(plain.poses) and all(np.array_equal(a, b) for a, b in zip(run.poses, plain.poses))
    assert len(run.factors) == len(plain.factors)
    for f, g in zip(run.factors, plain.factors):
        assert len(f) == len(g)
        assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(f, g))
    assert [(c.match_frame, c.query_frame) for c in run.closures] == [(c.match_frame, c.query_frame) for c in plain.closures]
    assert np.array_equal(run.cells, plain.cells) and len(run.cells) == run.live.n_hit_cells
    assert np.array_equal(run.published_map.view(np.uint64), plain.published_map.view(np.uint64))
    gm.close()
    gm2.close()
