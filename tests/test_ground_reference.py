"""scripts/ground_ref.py, the CPU restatement the device's ground segmentation is held to (tests/test_gpu_ground.py),
against labels worked out by hand on small scans; and what the labels are for: on a drive up a 6 % ramp the band on
world z marks the road itself as hit cells, the labels do not.  Runs on the CPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import ground_ref  # noqa: E402
import map_ref  # noqa: E402
from lidar_slam_from_scratch_amd import synth  # noqa: E402

G, O, I = ground_ref.GROUND, ground_ref.OBSTACLE, ground_ref.IGNORED
ROAD = -1.73

# a grid that is easy to work by hand: rings 1 m deep with centres at r + 0.5, four sectors, the quadrants in the order
# (-, -), (+, -), (+, +), (-, +); the other fields are the defaults: lim = 0.1 + 0.15 * (rc - gr)
SMALL = dict(n_rings=8, n_sectors=4, min_range=0.0, max_range=8.0)


def _at(ring, quadrant, z):
    """a row in `ring` of SMALL's grid, in the sector of `quadrant` (2: x, y > 0; 1: x > 0 > y)"""
    sy = {2: 1.0, 1: -1.0}[quadrant]
    return [ring + 0.3, 0.2 * sy, z]


def _bin(ring, quadrant):
    return ring * 4 + quadrant


def test_defaults_and_checks():
    assert ground_ref.DEFAULTS == dict(n_rings=80, n_sectors=180, min_range=0.5, max_range=80.5, sensor_height=1.73,
                                       max_slope=0.15, step_tol=0.1, height_tol=0.2, clear_min=0.3, clear_max=2.0)
    rows = np.array([_at(r, 2, ROAD) for r in range(8)] + [_at(r, 1, ROAD) for r in range(8)])
    b, q = ground_ref.bins_of(rows, dict(ground_ref.DEFAULTS, **SMALL))
    assert b.tolist() == [_bin(r, 2) for r in range(8)] + [_bin(r, 1) for r in range(8)]
    empty = ground_ref.segment(np.zeros((0, 3)), **SMALL)
    assert empty.counts() == (0, 0, 0, 0) and np.all(empty.ground_z == ROAD) and empty.sector_margin == float("inf")


def test_flat_ground_with_a_post():
    ground = [_at(r, 2, ROAD) for r in range(8)]
    post = [[5.3, 0.25, ROAD + h] for h in (0.1, 0.25, 0.31, 1.0, 1.99, 2.1)]      # in ring 5 with ground[5]
    res = ground_ref.segment(np.array(ground + post), **SMALL)
    # h <= 0.2 ground; (0.2, 0.3) neither; [0.3, 2.0] obstacle; above: neither
    assert res.labels.tolist() == [G] * 8 + [G, I, O, O, O, I]
    assert res.counts() == (9, 3, 2, 8)
    assert np.allclose(res.height[8:], [0.1, 0.25, 0.31, 1.0, 1.99, 2.1], atol=1e-12) and np.all(res.height[:8] == 0.0)
    assert np.all(res.ground_z == ROAD)                          # the other sectors keep the prior
    assert 0.0 < res.sector_margin < 0.5


def test_a_step_higher_than_lim_is_not_accepted():
    # rings 0..2 on the road; every return of ring 3 on a platform 0.5 m up: lim = 0.1 + 0.15 * (3.5 - 2.5) = 0.25
    rows = [_at(r, 2, ROAD) for r in range(3)] + [_at(3, 2, ROAD + 0.5), [3.6, 0.1, ROAD + 0.6]] + [_at(4, 2, ROAD)]
    res = ground_ref.segment(np.array(rows), **SMALL)
    assert res.labels.tolist() == [G, G, G, O, O, G]
    assert res.ground_z[_bin(3, 2)] == ROAD and res.bins_accepted == 4
    # the same platform 0.2 m up is within lim: it is ground, and the ground follows it
    rows[3][2], rows[4][2] = ROAD + 0.2, ROAD + 0.3
    res = ground_ref.segment(np.array(rows), **SMALL)
    assert res.labels.tolist() == [G, G, G, G, G, G] and res.ground_z[_bin(3, 2)] == ROAD + 0.2
    assert res.ground_z[_bin(4, 2)] == ROAD and res.bins_accepted == 5     # 0.2 down over one ring: within lim again


def test_lim_grows_over_empty_rings():
    # sector (+, +): ground in rings 0, 1, nothing in 2..4, ring 5 0.6 m up: lim = 0.1 + 0.15 * (5.5 - 1.5) = 0.7
    # sector (+, -): the same rise in ring 2: lim = 0.1 + 0.15 * (2.5 - 1.5) = 0.25
    far = [_at(0, 2, ROAD), _at(1, 2, ROAD), _at(5, 2, ROAD + 0.6)]
    near = [_at(0, 1, ROAD), _at(1, 1, ROAD), _at(2, 1, ROAD + 0.6)]
    res = ground_ref.segment(np.array(far + near), **SMALL)
    assert res.labels.tolist() == [G, G, G, G, G, O]
    gz = res.ground_z.reshape(8, 4)
    assert gz[:5, 2].tolist() == [ROAD] * 5 and gz[5:, 2].tolist() == [ROAD + 0.6] * 3   # inherited over the gap, then followed
    assert gz[:, 1].tolist() == [ROAD] * 8
    assert res.bins_accepted == 5
    # just past lim over the same gap: refused
    far[2][2] = ROAD + 0.71
    res = ground_ref.segment(np.array(far + near), **SMALL)
    assert res.labels[2] == O and res.ground_z.reshape(8, 4)[5, 2] == ROAD


def test_a_lone_low_return_does_not_drag_the_ground_down():
    rows = [_at(0, 2, ROAD), _at(1, 2, ROAD), _at(2, 2, ROAD), [2.6, 0.1, ROAD - 1.0], _at(3, 2, ROAD), [3.6, 0.1, ROAD + 0.5]]
    res = ground_ref.segment(np.array(rows), **SMALL)
    gz = res.ground_z.reshape(8, 4)
    # ring 2's minimum is the low return, 1 m off: refused (lim 0.25), so ring 2 inherits the road and ring 3, tested
    # against ring 1 (lim = 0.1 + 0.15 * 2 = 0.4), is accepted at the road's height
    assert gz[:, 2].tolist() == [ROAD] * 8 and res.bins_accepted == 3
    assert res.labels.tolist() == [G, G, G, G, G, O]             # the low return is below the ground: GROUND; 0.5 m up: OBSTACLE
    assert res.height[3] == -1.0 and res.height[5] == 0.5
    # had it been accepted, ring 3 would have been an obstacle 1 m up: that is what the step test prevents
    loose = ground_ref.segment(np.array(rows), step_tol=1.0, **SMALL)
    assert loose.ground_z.reshape(8, 4)[2, 2] == ROAD - 1.0 and loose.labels[4] == G and loose.bins_accepted == 4


def test_minimum_does_not_depend_on_row_order_and_ignores_non_finite_rows():
    rng = np.random.default_rng(0)
    rows = rng.uniform(-30, 30, size=(500, 3))
    rows[:, 2] = rng.uniform(-2.5, 2.0, size=500)
    rows[7] = [np.nan, 1.0, 0.0]
    rows[8] = [1.0, np.inf, 0.0]
    rows[9] = [1.0, 1.0, -np.inf]
    rows[10] = [0.1, 0.1, ROAD]                                  # inside min_range
    rows[11] = [80.0, 80.0, ROAD]                                # outside max_range
    a = ground_ref.segment(rows)
    p = rng.permutation(500)
    b = ground_ref.segment(rows[p])
    assert np.array_equal(a.labels[p], b.labels) and a.ground_z.tobytes() == b.ground_z.tobytes()
    assert np.all(a.labels[7:12] == I) and np.all(np.isnan(a.height[7:12])) and a.counts() == b.counts()


def test_ramp_ordering_and_rates():
    """The ramp drive, small: 16 beams x 360 azimuths, 12 frames, true poses.  Hit cells that hold no object return:
    what the band on world z adds, and the labels do not.  Measured on this scene: the band marks 7503
    cells, 6142 of them without an object return; the labels 1661 and 0; ground recall 49333 / 49333 = 1.0; object
    returns at least 0.5 m above the road labelled ground: 876 of 16558 = 0.0529 (with 16 beams many far bins hold
    object returns alone, and a wall's lowest return after a gap of empty rings passes for ground).  The bounds below
    are those figures with a margin of one point of recall and half as many leaks again."""
    grid = dict(resolution=0.2, height_min=0.3, height_max=2.0, max_range=40.0)
    opened = dict(grid, height_min=-sys.float_info.max, height_max=sys.float_info.max)
    band, band_obj, lab, lab_obj = set(), set(), set(), set()
    n_road = n_road_ground = n_high = n_high_ground = 0
    margin = 1.0
    for f in range(12):
        pts, is_object, T = synth.ramp_frame(f, 12, beams=16, azimuths=360)
        res = ground_ref.segment(pts)
        margin = min(margin, res.sector_margin)
        world = map_ref.world_points(pts, T)
        over_road = world[:, 2] - synth.ramp_road_z(world[:, 0])
        assert np.all(np.abs(over_road[~is_object]) < 1e-9) and over_road[is_object].min() > -1e-9
        high = is_object & (over_road >= 0.5)
        n_road += int((~is_object).sum())
        n_road_ground += int((~is_object & (res.labels == G)).sum())
        n_high += int(high.sum())
        n_high_ground += int((high & (res.labels == G)).sum())

        def cells(mask, g):
            return set(map(tuple, map_ref.hit_cells(world[mask], T[:2, 3], **g).tolist()))
        band |= cells(np.ones(len(pts), dtype=bool), grid)
        band_obj |= cells(is_object, grid)
        lab |= cells(res.labels == O, opened)
        lab_obj |= cells((res.labels == O) & is_object, opened)
    print("band: %d hit cells, %d without an object return; labels: %d, %d; ground recall %d / %d; object returns >= 0.5 m "
          "labelled ground %d / %d; sector margin %.3g" % (len(band), len(band - band_obj), len(lab), len(lab - lab_obj),
                                                          n_road_ground, n_road, n_high_ground, n_high, margin))
    assert margin >= 1e-9                                        # no beam lies on a sector's edge
    assert len(band - band_obj) > 0
    assert len(lab - lab_obj) < len(band - band_obj)
    assert len(lab) > 1000                                       # ... and not by labelling nothing an obstacle
    assert n_road > 40000 and n_high > 10000
    assert n_road_ground >= 0.99 * n_road
    assert n_high_ground <= 0.08 * n_high
