"""scripts/map_ref.py's count restatement (MapRef.raycast_counts, the normative text of icpmi_map_raycast_counts) held
to a literal reading of the definition in include/icp_mi355x.h: a loop over frames and rays with bresenham() and dict
counters.  Also the three relations to MapRef.raycast.  Runs on the CPU; tests/test_gpu_counts.py then holds the device
to the restatement."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import map_ref  # noqa: E402
from map_ref import bresenham  # noqa: E402


def _pose(x, y, yaw=0.0):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:2, 3] = x, y
    return T


def literal_counts(ref, poses, grid=None):
    """the definition, read literally: ({cell: hits}, {cell: misses})"""
    g = map_ref.grid_kwargs(grid)
    hits, misses = {}, {}
    for cloud, T in zip(ref.clouds, poses):
        T = np.asarray(T, dtype=np.float64)
        s = (int(np.floor(T[0, 3] / g["resolution"])), int(np.floor(T[1, 3] / g["resolution"])))
        H = set(map(tuple, map_ref.hit_cells(map_ref.world_points(cloud, T), T[:2, 3], **g).tolist()))
        carved = set()
        for hx, hy in H:
            carved.update(bresenham(s[0], s[1], hx, hy))
        for c in H:
            hits[c] = hits.get(c, 0) + 1
        for c in carved - H:
            misses[c] = misses.get(c, 0) + 1
    return hits, misses


def assert_literal(c, hits, misses, frames_used):
    """every field and every cell of a Counts against the two dicts"""
    observed = set(hits) | set(misses)
    if not observed:
        assert (c.min_x, c.min_y, c.width, c.height, c.n_observed, c.n_hit_cells, c.max_hits, c.max_misses) == (0,) * 8
        assert c.hits.shape == c.misses.shape == c.probability.shape == (0, 0)
        return
    xs, ys = [x for x, _ in observed], [y for _, y in observed]
    assert (c.min_x, c.min_y, c.width, c.height) == (min(xs) - 5, min(ys) - 5, max(xs) - min(xs) + 11, max(ys) - min(ys) + 11)
    assert (c.n_observed, c.n_hit_cells, c.frames_used) == (len(observed), len(hits), frames_used)
    assert (c.max_hits, c.max_misses) == (max(hits.values(), default=0), max(misses.values(), default=0))
    assert c.hits.dtype == c.misses.dtype == np.uint16 and c.probability.dtype == np.int8
    assert c.hits.shape == c.misses.shape == c.probability.shape == (c.height, c.width)
    want_h, want_m = np.zeros_like(c.hits), np.zeros_like(c.misses)
    want_p = np.full(c.probability.shape, -1, dtype=np.int8)
    for (x, y) in observed:
        h, m = hits.get((x, y), 0), misses.get((x, y), 0)
        want_h[y - c.min_y, x - c.min_x], want_m[y - c.min_y, x - c.min_x] = h, m
        want_p[y - c.min_y, x - c.min_x] = (200 * h + h + m) // (2 * (h + m))
    assert np.array_equal(c.hits, want_h) and np.array_equal(c.misses, want_m) and np.array_equal(c.probability, want_p)


def assert_relations(c, r):
    """hits > 0 <=> the raster is 100; hits == 0 and misses > 0 <=> it is 0; otherwise both are -1; one box"""
    assert (c.min_x, c.min_y, c.width, c.height, c.resolution) == (r.min_x, r.min_y, r.width, r.height, r.resolution)
    assert np.array_equal(c.hits > 0, r.data == 100)
    assert np.array_equal((c.hits == 0) & (c.misses > 0), r.data == 0)
    assert np.array_equal(c.probability == -1, r.data == -1)
    assert c.n_hit_cells == r.n_occupied and c.n_observed == r.n_occupied + r.n_free


def _random_store(seed, frames=5, rows=400):
    rng = np.random.default_rng(seed)
    ref, poses = map_ref.MapRef(), []
    for k in range(frames):
        c = rng.uniform(-25.0, 25.0, size=(rows, 3))
        c[:, 2] = rng.uniform(-1.0, 3.0, size=rows)
        ref.add_frame(c)
        poses.append(_pose(1.5 * k - 3.0, 1.0 * np.sin(k) - 0.5, 0.2 * k))
    return ref, poses


@pytest.mark.parametrize("seed,grid", [(3, None), (4, dict(resolution=1.0)), (5, dict(resolution=0.5, max_range=12.0))])
def test_literal_reading_on_small_stores(seed, grid):
    ref, poses = _random_store(seed)
    g = dict(map_ref.grid_kwargs(None), **(grid or {}))
    hits, misses = literal_counts(ref, poses, g)
    c = ref.raycast_counts(poses, g)
    assert set(hits) & set(misses) and max(hits.values()) > 1 and max(misses.values()) > 1   # what the store must exercise
    assert_literal(c, hits, misses, len(poses))
    assert_relations(c, ref.raycast(poses, g))
    # fewer poses than frames, and extra poses
    assert_literal(ref.raycast_counts(poses[:3], g), *literal_counts(ref, poses[:3], g), 3)
    assert_literal(ref.raycast_counts(poses + poses[:2], g), hits, misses, len(poses))


def test_a_frame_adds_at_most_one_and_the_rounding_tie():
    ref = map_ref.MapRef()
    ref.add_frame(np.tile([[10.05, 0.05, 1.0]], (1500, 1)))               # frame 0: one hit cell, 1,500 times
    for _ in range(7):
        ref.add_frame(np.array([[20.05, 0.05, 1.0]]))                     # frames 1-7 see through it
    poses = [_pose(0.05, 0.05)] * 8
    c = ref.raycast_counts(poses)
    at = lambda x, y: (int(c.hits[y - c.min_y, x - c.min_x]), int(c.misses[y - c.min_y, x - c.min_x]),  # noqa: E731
                       int(c.probability[y - c.min_y, x - c.min_x]))
    assert at(50, 0) == (1, 7, 13)                                        # 12.5 rounds half up
    assert at(100, 0) == (7, 0, 100) and at(0, 0) == (0, 8, 0) and at(101, 0) == (0, 0, -1)
    assert int(np.count_nonzero(c.misses)) == 100 and (c.n_observed, c.n_hit_cells, c.max_hits, c.max_misses) == (101, 2, 7, 8)
    assert_literal(c, *literal_counts(ref, poses), 8)
    assert_relations(c, ref.raycast(poses))
    p = map_ref.Counts.probability_of([0, 1, 1, 1, 2, 65535, 0], [3, 7, 2, 1, 1, 0, 0])
    assert p.tolist() == [0, 13, 33, 50, 67, 100, -1]


def test_within_one_scan_occupied_wins_but_not_across_scans():
    ref = map_ref.MapRef()
    ref.add_frame(np.array([[3.05, 0.05, 1.0], [10.05, 0.05, 1.0]]))      # frame 0 hits (15, 0) and, through it, (50, 0)
    ref.add_frame(np.array([[10.05, 0.05, 1.0]]))                         # frame 1 only looks through (15, 0)
    poses = [_pose(0.05, 0.05)] * 2
    assert (15, 0) in bresenham(0, 0, 50, 0)
    c = ref.raycast_counts(poses)
    assert (c.hits[0 - c.min_y, 15 - c.min_x], c.misses[0 - c.min_y, 15 - c.min_x]) == (1, 1)
    assert c.probability[0 - c.min_y, 15 - c.min_x] == 50 and ref.raycast(poses).data[0 - c.min_y, 15 - c.min_x] == 100
    assert_literal(c, *literal_counts(ref, poses), 2)


def test_refusals_and_nothing_observed():
    ref, poses = _random_store(6, frames=2, rows=50)
    for bad in (dict(resolution=0.0), dict(resolution=-1.0), dict(resolution=np.nan), dict(resolution=0.001, max_range=5.0),
                dict(max_range=np.inf)):
        with pytest.raises(ValueError):
            ref.raycast_counts(poses, dict(map_ref.grid_kwargs(None), **bad))
    with pytest.raises(ValueError):
        ref.raycast_counts([_pose(0.0, 0.0), _pose(1e5, 1e5)])            # 10^5 m apart on both axes: too many cells
    with pytest.raises(ValueError):
        ref.raycast_counts([_pose(np.nan, 0.0)] * 2)
    many = map_ref.MapRef()
    many.clouds = [np.zeros((0, 3))] * (map_ref.Counts.MAX_FRAMES + 1)
    assert map_ref.Counts.MAX_FRAMES == 65535
    with pytest.raises(ValueError):
        many.raycast_counts([_pose(0.0, 0.0)] * (map_ref.Counts.MAX_FRAMES + 1))     # one used frame too many
    for c, used in ((map_ref.MapRef().raycast_counts([]), 0), (ref.raycast_counts([]), 0),
                    (ref.raycast_counts(poses, dict(map_ref.grid_kwargs(None), height_min=50.0, height_max=60.0)), 2)):
        assert_literal(c, {}, {}, used)
        assert c.frames_used == used and c.resolution == 0.2
