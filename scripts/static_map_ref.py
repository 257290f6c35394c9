"""scripts/static_map_ref.py -- the CPU restatement of the static map (icpmi_map_world_static, icpmi_map_finish_static,
icpmi_map_static_labels; csrc/static_map.h) that tests/test_gpu_static_map.py holds the device to, byte for
byte.  It imports map_ref and leaves it untouched: the counts are MapRef.raycast_counts', the hit test is hit_cells'.

For the used frames i < used = min(frames, len(poses)) and the caller's grid, let hits[c], misses[c] and probability[c]
be exactly what MapRef.raycast_counts(poses, grid) defines.  The contract (include/icp_mi355x.h and csrc/static_map.h
state it in the same words):
    A row of used frame i VOTES iff it marks a cell c under the rules the counts use: grid_cell_key of its world
    point with frame i's translation as the sensor and, while icpmi_map_set_ground is on, additionally its label is
    OBSTACLE and the band is open.  With n = hits[c] + misses[c] a row's label is
      0  kept, does not vote: ground rows, rows out of band or ring, non-finite rows, an unrepresentable quotient
      1  kept, votes
      2  dropped: the row votes, n >= rule.min_observations and probability[c] < rule.min_probability
    probability[c] = (200 hits[c] + n) / (2 n) in integer division.  A lookup that finds n == 0, or a cell outside
    the plane's box, keeps the row with label 1 (it cannot happen for a voting row).  min_probability == 0 drops
    nothing.  All integer: no dependence on the order of frames, rows or threads.

As a program it prints the table of DESIGN 7.17: on moving_car_drive(), what the rule drops of the moving car's rows, of
the parked cars' rows and of all other rows."""
import collections
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import map_ref  # noqa: E402
from map_ref import orc  # noqa: E402

MIN_PROBABILITY_DEFAULT, MIN_OBSERVATIONS_DEFAULT = 50, 3   # ICPMI_STATIC_MIN_PROBABILITY_DEFAULT, ..._OBSERVATIONS_DEFAULT
QUIET, VOTES, DROPPED = 0, 1, 2
GROUND_OBSTACLE = 0                                         # ICPMI_GROUND_OBSTACLE
DBL_MAX = float(np.finfo(np.float64).max)

StaticInfo = collections.namedtuple("StaticInfo", "rows voting dropped kept")   # icpmi_static_info, less `live`


def rule_of(rule):
    """(min_probability, min_observations) of a capi.StaticRule, a pair, or None (the defaults); what the library refuses
    with ICPMI_ERR_ARG raises ValueError"""
    if rule is None:
        p, n, reserved = MIN_PROBABILITY_DEFAULT, MIN_OBSERVATIONS_DEFAULT, 0
    elif hasattr(rule, "min_probability"):
        p, n, reserved = rule.min_probability, rule.min_observations, getattr(rule, "reserved", 0)
    else:
        p, n, reserved = rule[0], rule[1], (rule[2] if len(rule) > 2 else 0)
    if not 0 <= p <= 100:
        raise ValueError("min_probability must lie in [0, 100]")
    if n < 1:
        raise ValueError("min_observations must be at least 1")
    if reserved != 0:
        raise ValueError("reserved must be 0")
    return int(p), int(n)


def row_cells(world, sensor_xy, resolution, height_min, height_max, max_range):
    """map_ref.hit_cells with the rows kept apart: (marks: bool per row, cells: (rows, 2) int64, (0, 0) where a row marks
    nothing).  The same IEEE operations; the cells of the marking rows are checked against hit_cells itself."""
    w = np.asarray(world, dtype=np.float64).reshape(-1, 3)
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    with np.errstate(all="ignore"):
        dx, dy = x - sensor_xy[0], y - sensor_xy[1]
        r = np.sqrt(dx * dx + dy * dy)
        cx, cy = np.floor(x / resolution), np.floor(y / resolution)
        ok = ~((z < height_min) | (z > height_max)) & ~((r > max_range) | (r < 0.5))
        ok &= (np.abs(cx) <= 2147483646.0) & (np.abs(cy) <= 2147483646.0)
    cells = np.zeros((w.shape[0], 2), dtype=np.int64)
    cells[ok, 0], cells[ok, 1] = cx[ok].astype(np.int64), cy[ok].astype(np.int64)
    assert np.array_equal(cells[ok], map_ref.hit_cells(w, sensor_xy, resolution, height_min, height_max, max_range))
    return ok, cells


def _used(clouds, poses):
    return min(len(clouds), len(poses))


def counts_of(clouds, poses, grid, ground_labels=None):
    """(MapRef.raycast_counts of the store, the grid the rows are tested under).  With ground labels: the counts of a
    second store holding, frame by frame, only the OBSTACLE rows, under the open band (icpmi_map_set_ground)."""
    g = map_ref.grid_kwargs(grid)
    ref = map_ref.MapRef()
    for i, c in enumerate(clouds):
        c = np.asarray(c, dtype=np.float64).reshape(-1, 3)
        ref.add_frame(c if ground_labels is None else c[np.asarray(ground_labels[i]) == GROUND_OBSTACLE])
    if ground_labels is not None:
        g = dict(g, height_min=-DBL_MAX, height_max=DBL_MAX)
    return ref.raycast_counts(poses, g), g


def static_labels(clouds, poses, grid, rule, ground_labels=None):
    """-> (one uint8 array of labels per used frame, StaticInfo).  ground_labels: None (ground off), or per frame its
    icpmi_map_ground_labels bytes."""
    min_probability, min_observations = rule_of(rule)
    counts, g = counts_of(clouds, poses, grid, ground_labels)
    out, rows, voting, dropped = [], 0, 0, 0
    for i in range(_used(clouds, poses)):
        T = np.asarray(poses[i], dtype=np.float64).reshape(4, 4)
        with np.errstate(all="ignore"):                                 # non-finite rows mark nothing
            world = map_ref.world_points(clouds[i], T)
        votes, cells = row_cells(world, T[:2, 3], g["resolution"], g["height_min"], g["height_max"], g["max_range"])
        if ground_labels is not None:
            votes &= np.asarray(ground_labels[i]) == GROUND_OBSTACLE
        label = votes.astype(np.uint8)                                  # 0 or 1
        lx, ly = cells[:, 0] - counts.min_x, cells[:, 1] - counts.min_y
        inside = votes & (lx >= 0) & (lx < counts.width) & (ly >= 0) & (ly < counts.height)
        h = np.zeros(len(label), dtype=np.int64)
        m = np.zeros(len(label), dtype=np.int64)
        h[inside], m[inside] = counts.hits[ly[inside], lx[inside]], counts.misses[ly[inside], lx[inside]]
        n = h + m
        probability = (200 * h + n) // np.maximum(2 * n, 1)
        drop = inside & (n > 0) & (n >= min_observations) & (probability < min_probability)
        label[drop] = DROPPED
        out.append(label)
        rows, voting, dropped = rows + len(label), voting + int(votes.sum()), dropped + int(drop.sum())
    return out, StaticInfo(rows, voting, dropped, rows - dropped)


def world_static(clouds, poses, grid, rule, first=0, ground_labels=None):
    """icpmi_map_world_static -> (the kept world rows of frames [first, used), frame then row order; the labels of every
    used frame; StaticInfo)"""
    labels, info = static_labels(clouds, poses, grid, rule, ground_labels)
    used = _used(clouds, poses)
    parts = [map_ref.world_points(clouds[i], poses[i])[labels[i] != DROPPED] for i in range(min(first, used), used)]
    return (np.concatenate(parts) if parts else np.zeros((0, 3))), labels, info


def finish_static(clouds, poses, grid, rule, voxel=1.0, ground_labels=None):
    """icpmi_map_finish_static -> (voxel_downsample(kept world rows of all used frames, voxel), as MapRef.finish filters
    the whole global map; StaticInfo)"""
    kept, _, info = world_static(clouds, poses, grid, rule, 0, ground_labels)
    published = orc.voxel_downsample(kept, voxel) if voxel > 0 and kept.shape[0] else np.zeros((0, 3))
    return published, info


# ------------------------------------------------------------------------------------------------ the moving-car drive

CAR_HALF = np.array([2.25, 0.9, 0.75])      # a 4.5 x 1.8 x 1.5 m box standing on the road (z = -1.73 .. -0.23)
CAR_PAD = 0.25                              # half a 0.5 m voxel: a centroid may mix a car's returns with its surroundings'
CAR_ROAD_CLEAR = 0.15                       # ... but a row this close to the road is the road's, beside or under the car
PARKED = ((-33.0, -3.0), (-20.0, -3.0))     # the parked cars' centres (x, y): 3 m beside the track, clear of the scene's boxes
MOVING_START, MOVING_STEP, MOVING_Y = -18.0, -2.0, 2.9   # the oncoming car: x = start + step * frame, in the other lane


def _car_box(x, y):
    c = np.array([x, y, -1.73 + CAR_HALF[2]])
    return c - CAR_HALF, c + CAR_HALF


def _inside(world, box):
    """the box padded by CAR_PAD on x, on y and above, and cut CAR_ROAD_CLEAR above the road below"""
    lo, hi = box[0] - CAR_PAD, box[1] + CAR_PAD
    lo[2] = box[0][2] + CAR_ROAD_CLEAR
    return np.all((world >= lo) & (world <= hi), axis=1)


def moving_car_drive(frames=12, azimuths=600, voxel=0.5, resolution=0.2, beams=64):
    """synth.lidar_pose's drive through synth._scene(3) plus two parked car boxes and one oncoming car box that moves
    2 m per frame in the other lane -> (clouds: per frame its voxel-filtered scan in the sensor frame, poses: the true
    ones, grid: a dict with a band that holds the cars (-1.4 .. 0.5 on world z: the sensor is the origin and the roofs
    lie at z = -0.23), moving: per frame a bool per row, True where the row came from the moving car, parked: the same
    for the two parked cars).  A row came from a car if its world point lies in the car's box at that frame, padded
    by CAR_PAD = 0.25 m on x, on y and above, and at least CAR_ROAD_CLEAR = 0.15 m above the road: the road's own returns
    beside and under a car never vote and are not the car's."""
    from lidar_slam_from_scratch_amd import synth
    clouds, poses, moving, parked = [], [], [], []
    parked_boxes = [_car_box(x, y) for x, y in PARKED]
    for f in range(frames):
        car = _car_box(MOVING_START + MOVING_STEP * f, MOVING_Y)
        scene = synth._scene(3) + parked_boxes + [car]
        T = synth.lidar_pose(f)
        pts = synth._raycast(T[:3, 3], T[:3, :3], scene, beams=beams, azimuths=azimuths)
        rng = np.random.Generator(np.random.PCG64(1000 + f))           # synth.lidar_frame's noise
        r = np.linalg.norm(pts, axis=1, keepdims=True)
        pts = pts * (1.0 + rng.normal(0.0, 0.01, size=r.shape) / np.maximum(r, 1e-9))
        pts = synth.voxel_centroids(pts, voxel) if voxel else pts
        world = map_ref.world_points(pts, T)
        clouds.append(np.ascontiguousarray(pts))
        poses.append(T)
        moving.append(_inside(world, car))
        parked.append(np.any([_inside(world, b) for b in parked_boxes], axis=0))
    grid = dict(resolution=float(resolution), height_min=-1.4, height_max=0.5, max_range=40.0)
    return clouds, poses, grid, moving, parked


def drive_shares(clouds, poses, grid, rule, moving, parked, ground_labels=None):
    """what the rule does on a drive: a dict of counts, and the three shares the tests assert"""
    labels, info = static_labels(clouds, poses, grid, rule, ground_labels)
    lab, mov, par = np.concatenate(labels), np.concatenate(moving), np.concatenate(parked)
    other = ~mov & ~par
    d = lab == DROPPED
    out = dict(rows=info.rows, voting=info.voting, dropped=info.dropped,
               car_rows=int(mov.sum()), car_dropped=int((d & mov).sum()),
               parked_rows=int(par.sum()), parked_dropped=int((d & par).sum()),
               other_rows=int(other.sum()), other_dropped=int((d & other).sum()))
    out["car_share"] = out["car_dropped"] / max(out["car_rows"], 1)
    out["parked_kept_share"] = 1.0 - out["parked_dropped"] / max(out["parked_rows"], 1)
    out["other_share"] = out["other_dropped"] / max(info.rows, 1)       # of all rows
    return out


def main():
    import ground_ref
    rules = ((MIN_PROBABILITY_DEFAULT, MIN_OBSERVATIONS_DEFAULT), (34, 3), (50, 6))
    print("moving_car_drive(): 12 frames, azimuths=600, voxel 0.5; band -1.4 .. 0.5, max_range 40")
    print("| votes by | resolution | rule (p, n) | rows | voting | car rows | car dropped | parked rows | parked dropped | "
          "other dropped | car share | other / all rows | other / voting |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for resolution in (0.2, 0.5):
        clouds, poses, grid, moving, parked = moving_car_drive(resolution=resolution)
        ground = [ground_ref.segment(c).labels for c in clouds]
        for name, gl in (("band", None), ("set_ground", ground)):
            for rule in rules:
                s = drive_shares(clouds, poses, grid, rule, moving, parked, gl)
                print("| %s | %.1f | (%d, %d) | %d | %d | %d | %d | %d | %d | %d | %.3f | %.4f | %.4f |"
                      % (name, resolution, rule[0], rule[1], s["rows"], s["voting"], s["car_rows"], s["car_dropped"],
                         s["parked_rows"], s["parked_dropped"], s["other_dropped"], s["car_share"], s["other_share"],
                         s["other_dropped"] / max(s["voting"], 1)))


if __name__ == "__main__":
    main()
