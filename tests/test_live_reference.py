"""scripts/map_ref.py's MapRefLive, the CPU restatement of icpmi_map_live_update (the decision of what to cast again,
and per-frame H_i and C_i added into counts that persist), held to MapRef.raycast_counts after every step of a sequence
that adds frames, moves a pose, drops poses and changes the grid, with frames_cast and rebuilt checked at each step.
Runs on the CPU (no device needed)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import map_ref  # noqa: E402


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-30.0, 30.0, size=(n, 3))
    c[:, 2] = rng.uniform(-0.5, 2.5, size=n)                              # some rows outside the height band
    return c


def _pose(x, y, yaw):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:2, 3] = [x, y]
    return T


def _info(c):
    return (c.min_x, c.min_y, c.width, c.height, c.resolution, c.n_observed, c.n_hit_cells, c.max_hits, c.max_misses,
            c.frames_used)


def _assert_equal(got, want):
    assert _info(got) == _info(want)
    for a, b in ((got.hits, want.hits), (got.misses, want.misses), (got.probability, want.probability)):
        assert a.dtype == b.dtype and a.shape == b.shape == (want.height, want.width) and np.array_equal(a, b)


GRID = dict(resolution=0.5, height_min=0.0, height_max=2.0, max_range=20.0)   # R = 40: quick on the CPU


def test_live_equals_batch_after_every_step():
    ref = map_ref.MapRefLive()
    sizes = [300, 0, 1, 700, 450, 5, 600]
    poses = [_pose(-6.0 + 2.5 * k, 3.0 - 1.5 * k, 0.3 * k) for k in range(len(sizes))]   # cells of both signs

    def step(P, grid, frames_cast, rebuilt):
        assert ref.live_update(P, grid) == (frames_cast, rebuilt)
        want = ref.raycast_counts(P, grid)
        _assert_equal(ref.live_counts(), want)
        return want

    assert _info(ref.live_counts()) == (0, 0, 0, 0, 0.0, 0, 0, 0, 0, 0)  # before any update
    step([], GRID, 0, 0)                                                  # no frame, no pose
    for k, n in enumerate(sizes):                                         # frames arrive one at a time
        ref.add_frame(_cloud(n, 100 + k))
        want = step(poses[:k + 1], GRID, 1, 0)
    assert want.max_hits > 1 and want.max_misses > 2 and int(np.count_nonzero((want.hits > 0) & (want.misses > 0))) > 0
    step(poses, GRID, 0, 0)                                               # nothing new
    step(poses + poses[:2], GRID, 0, 0)                                   # more poses than frames: nothing new either
    moved = [p.copy() for p in poses]
    moved[2][0, 3] = np.nextafter(moved[2][0, 3], np.inf)                 # one bit of one cast pose
    step(moved, GRID, 7, 1)
    step(moved[:4], GRID, 4, 1)                                           # fewer poses than were cast
    step(moved[:6], GRID, 2, 0)                                           # ... and more again: incremental from 4
    other = dict(GRID, resolution=0.25, max_range=10.0)                   # another grid
    step(moved[:6], other, 6, 1)
    ref.add_frame(_cloud(200, 200))
    ref.add_frame(_cloud(350, 201))
    P9 = moved + [_pose(9.0, -9.0, 1.0), _pose(11.0, -8.0, 1.2)]
    step(P9, other, 3, 0)                                                 # several frames at once
    ref.live_clear()
    assert _info(ref.live_counts()) == (0, 0, 0, 0, 0.0, 0, 0, 0, 0, 0)
    step(P9, other, 9, 0)                                                 # after a clear: everything, not "rebuilt"
    step([], other, 0, 1)                                                 # no poses at all: the counts are dropped


def test_refused_input_changes_nothing():
    ref = map_ref.MapRefLive()
    for k in range(3):
        ref.add_frame(_cloud(200, 300 + k))
    poses = [_pose(1.0 * k, -2.0 * k, 0.1) for k in range(3)]
    assert ref.live_update(poses[:2], GRID) == (2, 0)
    before = ref.live_counts()
    bad = [p.copy() for p in poses]
    bad[2][1, 1] = np.nan
    far = [p.copy() for p in poses]
    far[2][:2, 3] += 1e6
    for P, g in ((bad, GRID), (far, GRID), (poses, dict(GRID, resolution=0.0)), (poses, dict(GRID, max_range=np.inf)),
                 (poses, dict(GRID, resolution=0.001))):
        with pytest.raises(ValueError):
            ref.live_update(P, g)
        _assert_equal(ref.live_counts(), before)
    assert ref.live_update(poses, GRID) == (1, 0)                         # still incremental
    _assert_equal(ref.live_counts(), ref.raycast_counts(poses, GRID))
