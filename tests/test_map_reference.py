"""scripts/map_ref.py -- the CPU restatement of the node's map side that tests/test_gpu_map.py holds the device to --
checked against a literal, point-by-point Python reading of slam_node.cpp's loops (rebuild_recent_clouds :187-194,
build_final_global_map :196-209, update_occupancy_grid :211-221, rebuild_occupancy_grid :223-229,
publish_global_map :235-238) on small clouds.  Runs on the CPU."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import map_ref  # noqa: E402
from lidar_slam_from_scratch_amd import synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402

GRID = dict(resolution=0.2, height_min=0.3, height_max=2.0, max_range=40.0)   # slam_node.hpp:35-40
MAX_RECENT_CLOUDS = 20                                                         # slam_node.hpp:169


# ---- the node's loops, one point at a time --------------------------------------------------------------------------
def node_point(T, p):
    """poses_[i].R() * p + poses_[i].t(), row a: ((R_a0 x + R_a1 y) + R_a2 z) + t_a"""
    return [((float(p[0]) * T[a][0] + float(p[1]) * T[a][1]) + float(p[2]) * T[a][2]) + T[a][3] for a in range(3)]


def node_recent_clouds(clouds, poses):
    out = []                                                                   # recent_clouds_world_.clear()
    start = len(clouds) - MAX_RECENT_CLOUDS if len(clouds) > MAX_RECENT_CLOUDS else 0
    i = start
    while i < len(clouds) and i < len(poses):
        out.append([node_point(poses[i], p) for p in clouds[i]])
        i += 1
    return out


def node_global_map(clouds, poses):
    rows = []
    i = 0
    while i < len(clouds) and i < len(poses):
        for p in clouds[i]:
            rows.append(node_point(poses[i], p))
        i += 1
    return rows


def node_update_occupancy_grid(cells, cloud, sensor, g):
    for x, y, z in cloud:
        if z < g["height_min"] or z > g["height_max"]:
            continue
        r = math.sqrt((x - sensor[0]) * (x - sensor[0]) + (y - sensor[1]) * (y - sensor[1]))
        if r > g["max_range"] or r < 0.5:
            continue
        cells.add((int(math.floor(x / g["resolution"])), int(math.floor(y / g["resolution"]))))


def node_rebuild_occupancy_grid(clouds, poses, g):
    cells = set()                                                              # occupied_cells_.clear()
    i = 0
    while i < len(clouds) and i < len(poses):
        w = [node_point(poses[i], p) for p in clouds[i]]
        node_update_occupancy_grid(cells, w, [poses[i][0][3], poses[i][1][3], poses[i][2][3]], g)
        i += 1
    return cells


# ---- fixtures --------------------------------------------------------------------------------------------------------
def _clouds(F, rng, sizes=None):
    out = []
    for k in range(F):
        n = sizes[k] if sizes is not None else int(rng.integers(5, 60))
        c = rng.uniform(-15.0, 15.0, size=(n, 3))
        c[:, 2] = rng.uniform(-1.0, 3.0, size=n)
        out.append(c)
    return out


def _poses(F, rng):
    P = []
    for k in range(F):
        T = synth.make_transform(rng.uniform(-0.3, 0.3, size=3), np.array([0.7 * k, 0.1 * k, 0.02 * k]))
        P.append(T)
    return P


def _ref(clouds):
    m = map_ref.MapRef()
    for c in clouds:
        m.add_frame(c)
    return m


def _same_rows(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 3)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _row_bits(a):
    """rows as bit patterns, sorted: equal results for equal sets of rows"""
    u = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3).view(np.uint64)
    return u[np.lexsort(u.T[::-1])]


@pytest.mark.parametrize("F", [1, 7, 20, 21, 33])
@pytest.mark.parametrize("poses_short", [0, 3])
def test_restatement_matches_the_node(F, poses_short):
    rng = np.random.default_rng(1000 + F + 7 * poses_short)
    sizes = [int(rng.integers(5, 60)) for _ in range(F)]
    if F > 3:
        sizes[2] = 0                                   # an empty frame
    clouds = _clouds(F, rng, sizes)
    poses = _poses(F, rng)[:max(0, F - poses_short)]   # fewer poses than frames: those frames are not used
    m = _ref(clouds)
    lists = [T.tolist() for T in poses]
    recent = m.recent_clouds(poses)
    node_recent = node_recent_clouds(clouds, lists)
    assert len(recent) == len(node_recent)
    for a, b in zip(recent, node_recent):
        assert _same_rows(a, b)
    assert _same_rows(m.world(poses), node_global_map(clouds, lists))
    cells, published = m.finish(poses, None, 1.0)
    node_cells = node_rebuild_occupancy_grid(clouds, lists, GRID)
    assert set(map(tuple, cells.tolist())) == node_cells
    assert cells.dtype == np.int32 and len(cells) == len(node_cells)
    g = np.array(node_global_map(clouds, lists), dtype=np.float64).reshape(-1, 3)
    expect = orc.voxel_downsample(g, 1.0) if len(g) else np.zeros((0, 3))
    assert np.array_equal(_row_bits(published), _row_bits(expect))


def test_first_and_too_few_points_frames_are_in_the_rebuilt_set():
    """rebuild_occupancy_grid (:223-229) inserts every kept frame; the per-frame path (update_occupancy_grid at :153)
    never inserts frame 0 (:69-72) or a too-few-points frame (:125-130).  The restatement follows the rebuild."""
    rng = np.random.default_rng(7)
    clouds = _clouds(6, rng, [40, 40, 3, 40, 40, 40])
    clouds[0] = np.array([[1.0, 1.0, 1.0]])            # cells only frames 0 and 2 mark, far from the others'
    clouds[2] = np.array([[-5.0, 10.0, 1.0], [-5.5, 10.0, 1.0], [-6.0, 10.0, 1.0]])
    poses = [np.eye(4) for _ in range(6)]
    poses[0][:3, 3] = [99.0, 99.0, 0.0]
    poses[2][:3, 3] = [-45.0, 0.0, 0.0]
    for k in (1, 3, 4, 5):
        poses[k][:3, 3] = [float(k), 0.0, 0.0]
    m = _ref(clouds)
    cells, _ = m.finish(poses, GRID, 1.0)
    got = set(map(tuple, cells.tolist()))
    per_frame = set()                                  # the node's per-frame inserts, min_points = 10
    for k in range(1, 6):
        if clouds[k].shape[0] >= 10:
            node_update_occupancy_grid(per_frame, map_ref.world_points(clouds[k], poses[k]).tolist(), poses[k][:3, 3], GRID)
    first = set()
    node_update_occupancy_grid(first, map_ref.world_points(clouds[0], poses[0]).tolist(), poses[0][:3, 3], GRID)
    small = set()
    node_update_occupancy_grid(small, map_ref.world_points(clouds[2], poses[2]).tolist(), poses[2][:3, 3], GRID)
    assert first and small
    assert first <= got and small <= got
    assert not (first & per_frame) and not (small & per_frame)
    assert got == per_frame | first | small


def test_empty_store_and_no_poses():
    m = map_ref.MapRef()
    cells, published = m.finish([], None, 1.0)
    assert cells.shape == (0, 2) and published.shape == (0, 3)
    m.add_frame(np.zeros((0, 3)))
    m.add_frame(np.ones((4, 3)))
    assert m.world([]).shape == (0, 3)
    assert m.recent_clouds([np.eye(4)]) == [] or m.recent_clouds([np.eye(4)])[0].shape == (0, 3)
    assert m.size() == (2, 4)
