"""scripts/map_ref.py -- the CPU restatement of the node's map side (slam_viz/src/ros/slam_node.cpp:187-229, 235-238)
that tests/test_gpu_map.py holds the device (icpmi_map, lidar_slam_from_scratch_amd/global_map.py) to.

    downsampled_clouds_.push_back(curr)                                   :71, :123        add_frame
    rebuild_recent_clouds: frames [max(0, F - 20), F) moved by their pose :187-194         recent_clouds
    build_final_global_map: every frame moved by its final pose           :196-209         world(poses, 0)
    rebuild_occupancy_grid: clear, then update_occupancy_grid(world_i,    :223-229         finish -> cells
        poses[i].t()) for each frame
    publish_global_map once complete: voxel_downsample(global, voxel)     :235-238         finish -> published map

Only frames i < min(F, len(poses)) are used (the reference's i < downsampled_clouds_.size() && i < poses_.size()).
World points are ((x R_a0 + y R_a1) + z R_a2) + t_a, elementwise in numpy (no fused multiply-add), so they are the
device's bit for bit.  The cell set is the oracle's occupancy_update per frame, the published map its voxel_downsample.
The interface is GlobalMap's, so an instance can be handed to slam.run_slam as its global_map."""
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oracle import oracle as orc  # noqa: E402

MAX_RECENT_CLOUDS = 20   # slam_node.hpp:169


def world_points(cloud, pose):
    """cloud * R^T + t^T in the reference's summation order"""
    c = np.asarray(cloud, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(pose, dtype=np.float64).reshape(4, 4)
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    out = np.empty_like(c)
    for a in range(3):
        out[:, a] = ((x * T[a, 0] + y * T[a, 1]) + z * T[a, 2]) + T[a, 3]
    return out


def grid_kwargs(grid):
    """an icpmi_grid_config (capi.GridConfig), a dict, or None (OccupancyGridConfig's defaults)"""
    if grid is None:
        return dict(orc.GRID_DEFAULTS)
    if isinstance(grid, dict):
        return dict(grid)
    return {k: float(getattr(grid, k)) for k in orc.GRID_DEFAULTS}


def cells_array(cell_set):
    """a set of (x, y) -> (n, 2) int32 sorted by x then y (the order icpmi_occupancy_cells returns)"""
    return np.array(sorted(cell_set), dtype=np.int32).reshape(-1, 2)


class MapRef:
    def __init__(self):
        self.clouds = []

    def add_frame(self, cloud):
        self.clouds.append(np.ascontiguousarray(cloud, dtype=np.float64).reshape(-1, 3))

    def size(self):
        return len(self.clouds), int(sum(c.shape[0] for c in self.clouds))

    def world_frames(self, poses, first=0):
        last = min(len(self.clouds), len(poses))
        return [world_points(self.clouds[i], poses[i]) for i in range(first, last)]

    def world(self, poses, first=0):
        w = self.world_frames(poses, first)
        return np.concatenate(w) if w else np.zeros((0, 3))

    def recent_clouds(self, poses, max_recent=MAX_RECENT_CLOUDS):
        """rebuild_recent_clouds (:187-194): one world cloud per frame"""
        F = len(self.clouds)
        return self.world_frames(poses, F - max_recent if F > max_recent else 0)

    def cell_set(self, poses, grid=None):
        """rebuild_occupancy_grid (:223-229)"""
        g = grid_kwargs(grid)
        cells = set()                                                   # occupied_cells_.clear()
        for i, w in enumerate(self.world_frames(poses)):
            orc.occupancy_update(cells, w, np.asarray(poses[i], dtype=np.float64)[:3, 3], **g)
        return cells

    def finish(self, poses, grid=None, voxel=1.0):
        """(cells (n, 2) int32 sorted, voxel_downsample(global map, voxel)): build_final_global_map's tail"""
        cells = cells_array(self.cell_set(poses, grid))
        g = self.world(poses)
        published = orc.voxel_downsample(g, voxel) if voxel > 0 and g.shape[0] else np.zeros((0, 3))
        return cells, published
