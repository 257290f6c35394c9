"""The device's ground segmentation (icpmi_ground_segment, csrc/ground.h, lidar_slam_from_scratch_amd/ground.py)
against its CPU restatement (scripts/ground_ref.py, itself held to hand-worked scans by tests/test_ground_reference.py):
labels, height, ground_z and the counts byte for byte.  atan2 is the one step that is not exact arithmetic, so every
fixture's sector margin (the restatement reports it) is at least 1e-9; the two rows (-1, +-0.0, z) are exempt, they show
the sector wrap and its clamp.  Then the labels through the store (icpmi_map_set_ground): with ground set, each
occupancy product is byte for byte that of a second store holding only the OBSTACLE rows, run without ground and with an
open height band."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import torch  # noqa: F401  (first: one HIP runtime per process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import ground_ref  # noqa: E402
from lidar_slam_from_scratch_amd import capi, ground, slam, synth  # noqa: E402
from lidar_slam_from_scratch_amd.global_map import GlobalMap  # noqa: E402

pytestmark = pytest.mark.gpu

U8P = C.POINTER(C.c_uint8)
DBL_MAX = sys.float_info.max
MARGIN = 1e-9


@pytest.fixture()
def ctx():
    """Fails loudly (no skip, no fallback) when the HIP library or the device is missing."""
    from lidar_slam_from_scratch_amd import build
    build.build_library()
    c = capi.Context(device=0)
    yield c
    c.close()


def _cloud(n, seed, extent=60.0):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-extent, extent, size=(n, 3))
    c[:, 2] = rng.uniform(-2.5, 3.0, size=n)
    return c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(ctx, xyz, exempt=None, **cfg):
    """the device's result on xyz equals the restatement's in every byte; -> the restatement's result"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    want = ground_ref.segment(xyz, **cfg)
    margin = want.sector_margin if exempt is None else ground_ref.segment(xyz[~exempt], **cfg).sector_margin
    assert margin >= MARGIN, margin
    got = ground.ground_segment(ctx, xyz, ground.GroundConfig(**cfg))
    assert got.labels.dtype == np.uint8 and np.array_equal(got.labels, want.labels)
    assert np.array_equal(_bits(got.height), _bits(want.height))
    assert np.array_equal(_bits(got.ground_z).ravel(), _bits(want.ground_z))
    assert got.counts() == want.counts()
    return want


def test_empty_and_single(ctx):
    want = _check(ctx, np.zeros((0, 3)))
    assert want.counts() == (0, 0, 0, 0) and np.all(want.ground_z == -1.73)
    want = _check(ctx, [[10.0, 3.0, -1.7]])
    assert want.counts() == (1, 0, 0, 1)
    want = _check(ctx, [[1.0, 0.3, -0.7]])                      # 1.03 m over the prior, lim 0.25: an obstacle, no ground bin
    assert want.counts() == (0, 1, 0, 0)


def test_stride_and_labels(ctx):
    xyz = _cloud(1025, 1)                                       # one row past the workgroup's stride
    want = _check(ctx, xyz)
    assert min(want.n_ground, want.n_obstacle, want.n_ignored) > 50 and want.bins_accepted > 50
    _check(ctx, xyz[:1024])
    big = _check(ctx, _cloud(30000, 2))                         # many rows per bin
    assert big.bins_accepted > 1000


def test_one_bin_both_signs(ctx):
    rng = np.random.default_rng(3)
    z = rng.uniform(-1.0, 1.0, size=64)
    z[:4] = [0.0, -0.0, 5e-324, -5e-324]                        # the encoding's order around zero
    xyz = np.stack([10.0 + 1e-3 * rng.uniform(size=64), 0.1 + 1e-3 * rng.uniform(size=64), z], axis=1)
    b, _ = ground_ref.bins_of(xyz, ground_ref.DEFAULTS)
    assert len(set(b.tolist())) == 1 and b[0] >= 0
    for order in (np.arange(64), np.arange(64)[::-1], rng.permutation(64)):
        want = _check(ctx, xyz[order], sensor_height=0.9)
        assert want.bins_accepted == 1 and want.ground_z[b[0]] == z.min() and (z > 0).any() and z.min() < 0
    zero = xyz[:2].copy()                                        # +0.0 and -0.0 alone: the minimum is -0.0
    want = _check(ctx, zero, sensor_height=0.5)
    assert np.signbit(want.ground_z[b[0]])


def test_range_edges(ctx):
    cfg = dict(n_rings=5, n_sectors=7)                           # no sector edge on an axis but the wrap's
    lo, hi = 0.5, 80.5
    dn, up = np.nextafter(lo, 0.0), np.nextafter(hi, 100.0)
    rows = [(lo, 0, -1.7), (0, -lo, -1.7), (hi, 0, -1.0), (0, hi, -1.2),     # exactly on the limits: inside
            (dn, 0, -1.7), (0, -dn, -1.7), (up, 0, -1.0), (0, up, -1.2),     # the next doubles: outside
            (np.nextafter(lo, 1.0), 0, -1.6), (np.nextafter(hi, 0.0), 0, -1.1)]
    want = _check(ctx, rows, **cfg)
    assert np.array_equal(want.labels[4:8], [2, 2, 2, 2]) and np.all(np.isnan(want.height[4:8]))
    assert not np.any(np.isnan(want.height[[0, 1, 2, 3, 8, 9]]))
    b, _ = ground_ref.bins_of(np.array(rows, dtype=np.float64), dict(ground_ref.DEFAULTS, **cfg))
    assert b[0] // 7 == 0 and b[2] // 7 == 4                     # max_range itself falls in the last ring by the clamp


def test_sector_wrap(ctx):
    rows = np.array([(-1.0, 0.0, -1.7), (-1.0, -0.0, -1.5), (-1.0, 0.3, -1.6), (-1.0, -0.3, -1.4)])
    exempt = np.array([True, True, False, False])
    want = _check(ctx, rows, exempt=exempt)
    b, _ = ground_ref.bins_of(rows, ground_ref.DEFAULTS)
    assert b[0] == 179 and b[1] == 0                             # angle 2 pi is clamped into the last sector; angle 0
    assert want.ground_z[179] == -1.7 and want.ground_z[0] == -1.5


def test_non_finite_rows(ctx):
    xyz = _cloud(600, 4)
    bad = [np.nan, np.inf, -np.inf]
    for k, v in enumerate(bad * 3):
        xyz[5 + 7 * k, k // 3] = v
    xyz[100] = [np.nan, np.nan, np.nan]
    xyz[101] = [1e200, 1.0, 0.0]                                 # x * x overflows: out of range
    want = _check(ctx, xyz)
    assert np.all(want.labels[[5 + 7 * k for k in range(9)] + [100, 101]] == 2)


def test_grid_sizes(ctx):
    xyz = _cloud(3000, 5)
    one = _check(ctx, xyz, n_rings=1, n_sectors=1)
    assert one.ground_z.shape == (1,)
    assert capi.GROUND_MAX_BINS == ground_ref.MAX_BINS == 80 * 255
    full = _check(ctx, xyz, n_rings=80, n_sectors=255)           # every byte of LDS the kernel may ask for
    assert full.bins_accepted > 100
    _check(ctx, xyz, n_rings=capi.GROUND_MAX_BINS, n_sectors=1)
    _check(ctx, xyz, n_rings=1, n_sectors=1031)                  # more sectors than threads
    _check(ctx, xyz, n_rings=64, n_sectors=128)                  # exactly 64 KiB of bins: no attribute needed


def test_device_rows_and_null_outputs(ctx):
    xyz = _cloud(2000, 6)
    want = ground_ref.segment(xyz)
    d = torch.from_numpy(xyz).to("cuda:0")
    torch.cuda.synchronize()
    got = ground.ground_segment(ctx, None, device_ptr=d.data_ptr(), n_rows=2000)
    assert np.array_equal(got.labels, want.labels) and np.array_equal(_bits(got.height), _bits(want.height))
    assert got.counts() == want.counts()
    lib, cfg = capi.load_library(), ground.GroundConfig().to_c()
    labels = np.full(2000, 9, dtype=np.uint8)
    ctx._check(lib.icpmi_ground_segment(ctx._h, capi._dp(xyz), 2000, C.byref(cfg), labels.ctypes.data_as(U8P), None, None, None))
    assert np.array_equal(labels, want.labels)


def test_bad_configs_write_nothing(ctx):
    lib = capi.load_library()
    xyz = _cloud(100, 7)
    bad = [dict(n_rings=1, n_sectors=capi.GROUND_MAX_BINS + 1), dict(n_rings=capi.GROUND_MAX_BINS // 2 + 1, n_sectors=2),
           dict(n_rings=0), dict(n_sectors=0), dict(n_rings=-3), dict(n_rings=65536, n_sectors=65536),
           dict(min_range=-0.1), dict(max_range=0.5), dict(max_range=0.4), dict(max_slope=-1e-9), dict(step_tol=-1e-9),
           dict(height_tol=-1e-9), dict(clear_min=2.0, clear_max=1.9)]
    for name in ("min_range", "max_range", "sensor_height", "max_slope", "step_tol", "height_tol", "clear_min", "clear_max"):
        bad += [{name: np.nan}, {name: np.inf}, {name: -np.inf}]
    gm = GlobalMap(ctx)
    for kw in bad:
        with pytest.raises(ValueError):
            ground_ref.check(kw)
        cfg = ground.GroundConfig(**kw).to_c()
        labels, height, gz = np.full(100, 9, dtype=np.uint8), np.full(100, 7.0), np.full(64, 7.0)
        info = capi.GroundInfo(-1, -1, -1, -1)
        rc = lib.icpmi_ground_segment(ctx._h, capi._dp(xyz), 100, C.byref(cfg), labels.ctypes.data_as(U8P), capi._dp(height),
                                      capi._dp(gz), C.byref(info))
        assert rc == capi.ERR_ARG, kw
        assert np.all(labels == 9) and np.all(height == 7.0) and np.all(gz == 7.0)
        assert (info.n_ground, info.n_obstacle, info.n_ignored, info.bins_accepted) == (-1, -1, -1, -1)
        assert lib.icpmi_map_set_ground(gm._h, C.byref(cfg)) == capi.ERR_ARG
    with pytest.raises(capi.IcpError) as e:                      # no bad config was taken: ground is still off
        gm.ground_labels(0)
    assert e.value.code == capi.ERR_ARG
    gm.close()


# ---- through the store ----

def _grid(**kw):
    return capi.Context.make_grid_config(**kw)


def _open(grid):
    return _grid(resolution=grid.resolution, height_min=-DBL_MAX, height_max=DBL_MAX, max_range=grid.max_range)


def test_store_labels(ctx):
    rng = np.random.default_rng(8)
    sizes = [0, 1, 7, 1023, 1024, 1025, 0, 3000] + rng.integers(0, 2500, size=62).tolist()
    sizes[20] = sizes[21] = 0
    clouds = [_cloud(n, 100 + k) for k, n in enumerate(sizes)]
    gm = GlobalMap(ctx)
    gm.set_ground(ground.GroundConfig())
    for c in clouds[:40]:
        gm.add_frame(c)
    with pytest.raises(capi.IcpError) as e:
        gm.ground_labels(40)
    assert e.value.code == capi.ERR_ARG
    want = [ground.ground_segment(ctx, c).labels for c in clouds]
    assert np.array_equal(gm.ground_labels(39), want[39])        # labels frames 0 .. 39 in one launch
    for k, c in enumerate(clouds[40:]):                          # ... the rest in a second one, behind them
        if k % 2:
            d = torch.from_numpy(c).to("cuda:0")
            torch.cuda.synchronize()
            gm.add_frame_device(d.data_ptr() if len(c) else 0, len(c))
            del d
        else:
            gm.add_frame(c)
    assert len(sizes) == 70
    for k in reversed(range(70)):
        got = gm.ground_labels(k)
        assert got.shape == (sizes[k],) and np.array_equal(got, want[k]), k
    cfg2 = ground.GroundConfig(n_rings=20, n_sectors=60, height_tol=0.4)    # another config: labelled again
    gm.set_ground(cfg2)
    for k in (0, 5, 7, 69):
        assert np.array_equal(gm.ground_labels(k), ground.ground_segment(ctx, clouds[k], cfg2).labels)
    gm.set_ground(None)
    with pytest.raises(capi.IcpError) as e:
        gm.ground_labels(0)
    assert e.value.code == capi.ERR_ARG
    gm.close()


@pytest.fixture(scope="module")
def ramp():
    """a dozen frames of the ramp drive (16 beams x 360 azimuths), an empty frame and a frame of road returns alone
    (rows, but no OBSTACLE row) among them, with their true poses"""
    frames, poses = [], []
    for f in range(12):
        pts, _, T = synth.ramp_frame(f, 12, beams=16, azimuths=360)
        frames.append(pts)
        poses.append(T)
    frames[4] = np.zeros((0, 3))
    pts, is_object, _ = synth.ramp_frame(7, 12, beams=16, azimuths=360)
    frames[7] = pts[~is_object]
    return frames, poses


def _products(gm, ctx, poses, grid, updates):
    """the four products with their info fields, as comparable tuples; the live counts after live updates over
    poses[:k] for each k of `updates`"""
    cells, published = gm.finish(poses, grid)
    r = gm.raycast(poses, grid)
    c = gm.raycast_counts(poses, grid)
    log = []
    for k in updates:
        i = gm.live_update(poses[:k], grid)
        log.append((i.frames_cast, i.rebuilt, i.moved, i.plane_x0, i.plane_y0, i.plane_w, i.plane_h))
    lc, li = gm.live_counts()

    def counts(c):
        return (c.min_x, c.min_y, c.width, c.height, c.resolution, c.n_observed, c.n_hit_cells, c.max_hits, c.max_misses,
                c.frames_used, c.hits.tobytes(), c.misses.tobytes(), c.probability.tobytes())
    return dict(cells=cells.tobytes(), raster=(r.min_x, r.min_y, r.width, r.height, r.resolution, r.n_occupied, r.n_free,
                                               r.data.tobytes()),
                counts=counts(c), live=counts(lc), live_log=log), published, c


def test_store_equivalence(ctx, ramp):
    frames, poses = ramp
    cfg = ground.GroundConfig()
    gm, only = GlobalMap(ctx), GlobalMap(ctx)
    for f in frames:
        gm.add_frame(f)
    gm.set_ground(cfg)
    kept = []
    for k, f in enumerate(frames):
        lab = gm.ground_labels(k)
        assert np.array_equal(lab, ground.ground_segment(ctx, f, cfg).labels)
        kept.append(int((lab == ground.OBSTACLE).sum()))
        only.add_frame(f[lab == ground.OBSTACLE])                # the second store: the OBSTACLE rows, in order
    assert kept[4] == 0 and kept[7] == 0 and len(frames[7]) > 1000 and min(kept[:4]) > 300
    updates = (5, 8, 9, 12)                                      # the live plane: built, then grown frame by frame
    hit_cells = []
    for grid in (_grid(resolution=0.05, max_range=40.0), _grid(resolution=0.5, max_range=20.0), _grid()):
        gm.live_clear(), only.live_clear()                       # R = 800: windows in device scratch; 40, 200: in LDS
        got, published, c = _products(gm, ctx, poses, grid, updates)
        want, _, _ = _products(only, ctx, poses, _open(grid), updates)
        assert c.n_hit_cells > 100 and c.max_hits > 1
        hit_cells.append(c.n_hit_cells)
        for name in ("cells", "raster", "counts", "live", "live_log"):
            assert got[name] == want[name], (name, grid.resolution)
        assert got["live"] == got["counts"]
    # ground off again: the bytes from before the config; the published map never changed
    grid = _grid()
    plain = GlobalMap(ctx)
    for f in frames:
        plain.add_frame(f)
    want, want_pub, c_plain = _products(plain, ctx, poses, grid, updates)
    gm.live_clear()
    gm.set_ground(cfg)
    assert np.array_equal(_bits(gm.finish(poses, grid)[1]), _bits(want_pub))
    gm.set_ground(None)
    got, got_pub, _ = _products(gm, ctx, poses, grid, updates)
    assert got == want and np.array_equal(_bits(got_pub), _bits(want_pub))
    assert c_plain.n_hit_cells > hit_cells[-1]                   # the band took the climbing road for a wall
    for m in (gm, only, plain):
        m.close()


def test_all_frames_without_obstacles(ctx, ramp):
    """rows in the store, but no OBSTACLE row in any used frame: the empty products, as from a store of empty frames"""
    frames, poses = ramp
    gm, only = GlobalMap(ctx), GlobalMap(ctx)
    for _ in range(3):
        gm.add_frame(frames[7])
        only.add_frame(np.zeros((0, 3)))
    gm.set_ground(ground.GroundConfig())
    grid = _grid()
    got, _, _ = _products(gm, ctx, poses[:3], grid, (2, 3))
    want, _, _ = _products(only, ctx, poses[:3], _open(grid), (2, 3))
    assert got == want and got["counts"][2:4] == (0, 0)
    gm.close(), only.close()


def test_live_after_set_ground(ctx, ramp):
    frames, poses = ramp
    gm = GlobalMap(ctx)
    for f in frames[:6]:
        gm.add_frame(f)
    grid = _grid()
    i = gm.live_update(poses[:6], grid)
    assert (i.frames_cast, i.rebuilt) == (6, 0)
    cfg = ground.GroundConfig()
    gm.set_ground(cfg)
    i = gm.live_update(poses[:6], grid)
    assert (i.frames_cast, i.rebuilt) == (6, 1)
    gm.add_frame(frames[6])
    i = gm.live_update(poses[:7], grid)
    assert (i.frames_cast, i.rebuilt) == (1, 0)                  # incremental again; the new frame was labelled
    gm.set_ground(cfg)                                           # the same config: still a rebuild
    i = gm.live_update(poses[:7], grid)
    assert (i.frames_cast, i.rebuilt) == (7, 1)
    want = gm.raycast_counts(poses[:7], grid)
    got = gm.live_counts()[0]
    assert got.hits.tobytes() == want.hits.tobytes() and got.misses.tobytes() == want.misses.tobytes()
    gm.set_ground(None)
    i = gm.live_update(poses[:7], grid)
    assert (i.frames_cast, i.rebuilt) == (7, 1)
    gm.close()


def test_run_slam_ground(ctx, ramp):
    frames, _ = ramp
    frames = [f for k, f in enumerate(frames) if k not in (4, 7)]    # the scans of the drive itself
    cfg = ground.GroundConfig()
    gm = GlobalMap(ctx)
    run = slam.run_slam(frames, ctx, global_map=gm, counts=True, ground=cfg)
    direct = GlobalMap(ctx)
    for f in frames:
        direct.add_frame(f)
    direct.set_ground(cfg)
    want = direct.raycast_counts(run.poses)
    got = run.counts
    assert want.n_hit_cells > 100
    assert (got.min_x, got.min_y, got.width, got.height, got.n_observed, got.n_hit_cells, got.frames_used) == \
        (want.min_x, want.min_y, want.width, want.height, want.n_observed, want.n_hit_cells, want.frames_used)
    assert got.hits.tobytes() == want.hits.tobytes() and got.misses.tobytes() == want.misses.tobytes()
    assert got.probability.tobytes() == want.probability.tobytes()
    direct.set_ground(None)
    assert direct.raycast_counts(run.poses).hits.tobytes() != want.hits.tobytes()
    plain = slam.run_slam(frames, ctx, ground=cfg)               # ignored without a global_map
    assert plain.counts is None
    gm.close(), direct.close()
