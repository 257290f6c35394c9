"""scripts/map_ref.py's ray-cast restatement (MapRef.raycast, the normative text of icpmi_map_raycast) held to the
definition in include/icp_mi355x.h: the walk, occupied over free, the bounds, the rows that cast no ray.  Runs on the
CPU; tests/test_gpu_raycast.py then holds the device to the restatement."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import map_ref  # noqa: E402
from map_ref import bresenham, bresenham_lockstep  # noqa: E402


def _pose(x, y, yaw=0.0):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:2, 3] = x, y
    return T


def _lock(x0, y0, x1, y1):
    return set(map(tuple, bresenham_lockstep(x0, y0, x1, y1).tolist()))


def test_the_quoted_walks_and_direction():
    assert bresenham(0, 0, 5, 2) == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2)]
    assert bresenham(5, 2, 0, 0) == [(5, 2), (4, 2), (3, 1), (2, 1), (1, 0)]
    assert set(bresenham(0, 0, 5, 2)) != set(bresenham(5, 2, 0, 0))      # not symmetric: the direction is part of it
    assert bresenham(3, -4, 3, -4) == [] and len(bresenham_lockstep(3, -4, 3, -4)) == 0


def test_axis_diagonal_and_octant_rays():
    assert bresenham(2, 1, 6, 1) == [(2, 1), (3, 1), (4, 1), (5, 1)]
    assert bresenham(2, 1, -2, 1) == [(2, 1), (1, 1), (0, 1), (-1, 1)]
    assert bresenham(2, 1, 2, 4) == [(2, 1), (2, 2), (2, 3)]
    assert bresenham(2, 1, 2, -2) == [(2, 1), (2, 0), (2, -1)]
    for sx in (1, -1):
        for sy in (1, -1):
            assert bresenham(0, 0, 4 * sx, 4 * sy) == [(k * sx, k * sy) for k in range(4)]
    for ex, ey in ((7, 3), (3, 7), (-3, 7), (-7, 3), (-7, -3), (-3, -7), (3, -7), (7, -3)):     # one per octant
        cells = bresenham(0, 0, ex, ey)
        n = max(abs(ex), abs(ey))
        assert len(cells) == n and cells[0] == (0, 0) and (ex, ey) not in cells
        steps = np.diff(np.array(cells + [(ex, ey)]), axis=0)
        assert (np.abs(steps).max(axis=1) == 1).all()                    # 8-connected, one cell along the long axis
        long_axis = 0 if abs(ex) > abs(ey) else 1
        assert (steps[:, long_axis] == np.sign((ex, ey)[long_axis])).all()
        # never more than half a cell off the ideal line, measured along the short axis
        for k, c in enumerate(cells):
            ideal = (ex, ey)[1 - long_axis] * k / n
            assert abs(c[1 - long_axis] - ideal) <= 0.5
        assert _lock(0, 0, ex, ey) == set(cells)


def test_lockstep_equals_scalar_on_random_ends():
    rng = np.random.default_rng(7)
    ends = rng.integers(-210, 211, size=(500, 2))
    got = bresenham_lockstep(-3, 11, ends[:, 0], ends[:, 1])
    want = [c for ex, ey in ends.tolist() for c in bresenham(-3, 11, ex, ey)]
    assert len(got) == len(want)                                          # cell for cell, per ray
    assert sorted(map(tuple, got.tolist())) == sorted(want)


def test_occupied_wins_over_a_crossing_ray():
    ref = map_ref.MapRef()
    ref.add_frame(np.array([[3.05, 0.05, 1.0]]))                          # frame 0 at the origin: hits cell (15, 0)
    ref.add_frame(np.array([[10.05, 0.0, 1.0]]))                          # frame 1 from (-2, 0.05): hits (40, 0)
    poses = [_pose(0.0, 0.0), _pose(-2.0, 0.05)]
    assert (15, 0) in bresenham(-10, 0, 40, 0)                            # frame 1's ray crosses frame 0's hit cell
    r = ref.raycast(poses)
    assert r.cells(map_ref.OCCUPIED) == {(15, 0), (40, 0)} == ref.cell_set(poses)
    assert r.data[0 - r.min_y, 15 - r.min_x] == 100
    assert r.cells(map_ref.FREE) == (set(bresenham(0, 0, 15, 0)) | set(bresenham(-10, 0, 40, 0))) - {(15, 0)}
    assert r.n_occupied == 2 and r.n_free == 15 + 50 - 15 - 1             # the rays share (0..14, 0); (15, 0) is occupied


def test_bounds_and_the_empty_raster():
    ref = map_ref.MapRef()
    ref.add_frame(np.array([[3.05, 1.25, 1.0]]))
    r = ref.raycast([_pose(-0.3, -0.3)])                                  # sensor cell (-2, -2), hit cell (13, 4)
    assert (r.min_x, r.min_y, r.width, r.height) == (-2 - 5, -2 - 5, 13 + 2 + 11, 4 + 2 + 11)
    assert r.data.shape == (r.height, r.width) and r.data.dtype == np.int8
    assert r.data[4 - r.min_y, 13 - r.min_x] == 100 and r.data[-2 - r.min_y, -2 - r.min_x] == 0
    assert (r.data[:5] == -1).all() and (r.data[-5:] == -1).all() and (r.data[:, :5] == -1).all() and (r.data[:, -5:] == -1).all()
    assert r.resolution == 0.2
    for empty in (map_ref.MapRef().raycast([]), ref.raycast([])):         # no frame; no pose
        assert (empty.width, empty.height, empty.n_occupied, empty.n_free) == (0, 0, 0, 0) and empty.data.shape == (0, 0)
    # a hit in the sensor's own cell: occupied, nothing carved
    own = map_ref.MapRef()
    own.add_frame(np.array([[0.6, 0.0, 1.0]]))
    r = own.raycast([_pose(0.1, 0.1)], dict(map_ref.grid_kwargs(None), resolution=1.0))
    assert (r.n_occupied, r.n_free, r.width, r.height) == (1, 0, 11, 11)


def test_rows_out_of_band_or_range_carve_nothing():
    rows = np.array([[5.0, 0.0, 0.29], [5.0, 0.0, 2.01],                  # outside [height_min, height_max] = [0.3, 2]
                     [0.3, 0.3, 1.0], [40.1, 0.0, 1.0],                   # r < 0.5, r > max_range = 40
                     [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1e12, 0.0, 1.0]])
    ref = map_ref.MapRef()
    ref.add_frame(rows)
    r = ref.raycast([_pose(0.0, 0.0)])
    assert (r.width, r.height, r.n_occupied, r.n_free) == (0, 0, 0, 0)
    ref.add_frame(np.array([[1.0, 1.0, 1.0]]))
    r = ref.raycast([_pose(0.0, 0.0)] * 2)
    assert r.n_occupied == 1 and r.cells(map_ref.FREE) == set(bresenham(0, 0, 5, 5))
    for bad in (dict(resolution=0.0), dict(resolution=-1.0), dict(resolution=np.nan), dict(resolution=0.001, max_range=5.0),
                dict(max_range=np.inf)):
        with pytest.raises(ValueError):
            ref.raycast([_pose(0.0, 0.0)] * 2, dict(map_ref.grid_kwargs(None), **bad))
    with pytest.raises(ValueError):
        ref.raycast([_pose(0.0, 0.0), _pose(1e5, 1e5)])                   # 10^5 m apart on both axes: too many cells
    with pytest.raises(ValueError):
        ref.raycast([_pose(np.nan, 0.0)] * 2)


def _random_store(seed, frames=5, rows=400):
    rng = np.random.default_rng(seed)
    ref, poses = map_ref.MapRef(), []
    for k in range(frames):
        c = rng.uniform(-25.0, 25.0, size=(rows, 3))
        c[:, 2] = rng.uniform(-1.0, 3.0, size=rows)
        ref.add_frame(c)
        poses.append(_pose(3.0 * k - 6.0, 2.0 * np.sin(k) - 1.0, 0.2 * k))
    return ref, poses


def test_frame_order_does_not_matter_and_occupied_is_the_cell_set():
    ref, poses = _random_store(3)
    a = ref.raycast(poses)
    assert a.cells(map_ref.OCCUPIED) == ref.cell_set(poses) and a.n_occupied == len(ref.cell_set(poses))
    assert a.n_free > a.n_occupied > 0 and not (a.cells(map_ref.FREE) & a.cells(map_ref.OCCUPIED))
    back = map_ref.MapRef()
    for c in ref.clouds[::-1]:
        back.add_frame(c)
    b = back.raycast(poses[::-1])
    assert (a.min_x, a.min_y, a.width, a.height, a.n_occupied, a.n_free) == (b.min_x, b.min_y, b.width, b.height, b.n_occupied, b.n_free)
    assert np.array_equal(a.data, b.data)
    # the same raster from the scalar walk, ray by ray
    g = map_ref.grid_kwargs(None)
    occupied, carved = set(), set()
    for cloud, T in zip(ref.clouds, poses):
        s = (int(np.floor(T[0, 3] / 0.2)), int(np.floor(T[1, 3] / 0.2)))
        for hx, hy in map_ref.hit_cells(map_ref.world_points(cloud, T), T[:2, 3], **g).tolist():
            occupied.add((hx, hy))
            carved.update(bresenham(s[0], s[1], hx, hy))
    assert a.cells(map_ref.OCCUPIED) == occupied and a.cells(map_ref.FREE) == carved - occupied
    assert carved & occupied                                              # some ray does cross another's hit cell
