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
The interface is GlobalMap's, so an instance can be handed to slam.run_slam as its global_map.

MapRefLive restates icpmi_map_live_update: the decision of what to cast again, and counts that persist.

MapRef.raycast is the normative text of icpmi_map_raycast (include/icp_mi355x.h, csrc/raycast.h): the kept scans
ray-cast into a free / occupied / unknown raster.  bresenham() restates the device's ray_walk line for line;
bresenham_lockstep() is the same walk for many rays at once, one step per numpy operation."""
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


RAYCAST_MAX_R = 4096        # ICPMI_RAYCAST_MAX_R
UNKNOWN, FREE, OCCUPIED = -1, 0, 100


class Raster:
    """what icpmi_map_raster returns: the info fields, and data[y - min_y, x - min_x] as (height, width) int8"""

    def __init__(self, min_x, min_y, width, height, resolution, n_occupied, n_free, data):
        self.min_x, self.min_y, self.width, self.height = int(min_x), int(min_y), int(width), int(height)
        self.resolution, self.n_occupied, self.n_free = float(resolution), int(n_occupied), int(n_free)
        self.data = data

    def cells(self, value):
        """the (x, y) cells holding `value`, as a set"""
        y, x = np.nonzero(self.data == value)
        return set(zip((x + self.min_x).tolist(), (y + self.min_y).tolist()))


class Counts:
    """what icpmi_map_counts returns: the info fields, and hits, misses (uint16) and probability (int8), each
    [y - min_y, x - min_x] as (height, width)"""
    MAX_FRAMES = 65535      # ICPMI_RAYCOUNT_MAX_FRAMES: a count is 16 bits wide and a frame adds at most 1

    def __init__(self, min_x, min_y, width, height, resolution, n_observed, n_hit_cells, max_hits, max_misses,
                 frames_used, hits, misses, probability):
        self.min_x, self.min_y, self.width, self.height = int(min_x), int(min_y), int(width), int(height)
        self.resolution, self.n_observed, self.n_hit_cells = float(resolution), int(n_observed), int(n_hit_cells)
        self.max_hits, self.max_misses, self.frames_used = int(max_hits), int(max_misses), int(frames_used)
        self.hits, self.misses, self.probability = hits, misses, probability

    @staticmethod
    def probability_of(hits, misses):
        """-1 where hits + misses == 0; else (200 hits + n) // (2 n), n = hits + misses: 100 hits / n rounded half
        up, in integers"""
        h, m = np.asarray(hits, dtype=np.int64), np.asarray(misses, dtype=np.int64)
        n = h + m
        return np.where(n == 0, -1, (200 * h + n) // np.maximum(2 * n, 1)).astype(np.int8)


def bresenham(x0, y0, x1, y1):
    """ray_walk (csrc/raycast.h): the cells carved on the way from (x0, y0) to (x1, y1): the first, not the last"""
    out = []
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx = 1 if x1 > x0 else (-1 if x1 < x0 else 0)
    sy = 1 if y1 > y0 else (-1 if y1 < y0 else 0)
    err, x, y = dx - dy, x0, y0
    while x != x1 or y != y1:
        out.append((x, y))
        e2 = 2 * err
        if e2 > -dy:
            err -= dy
            x += sx
        if e2 < dx:
            err += dx
            y += sy
    return out


def bresenham_lockstep(x0, y0, x1, y1):
    """bresenham() for arrays of rays, all advanced one step per pass: the carved cells of all of them, (n, 2) int64
    (a cell once per ray that carves it, in no particular order).  Every pass moves a ray one cell along its longer
    axis, so a ray takes max(dx, dy) passes: with the rays sorted longest first, the live ones are a prefix."""
    x0, y0, x1, y1 = (np.asarray(a, dtype=np.int64).ravel() for a in np.broadcast_arrays(x0, y0, x1, y1))
    order = np.argsort(-np.maximum(np.abs(x1 - x0), np.abs(y1 - y0)), kind="stable")
    x0, y0, x1, y1 = x0[order], y0[order], x1[order], y1[order]
    dx, dy = np.abs(x1 - x0), np.abs(y1 - y0)
    sx, sy = np.sign(x1 - x0), np.sign(y1 - y0)
    err, x, y = dx - dy, x0.copy(), y0.copy()
    out = []
    n = int(np.count_nonzero((x != x1) | (y != y1)))
    while n:
        out.append(np.stack([x[:n], y[:n]], axis=1))
        e2 = 2 * err[:n]
        mx, my = e2 > -dy[:n], e2 < dx[:n]
        err[:n] += my * dx[:n] - mx * dy[:n]
        x[:n] += mx * sx[:n]
        y[:n] += my * sy[:n]
        n = int(np.count_nonzero((x[:n] != x1[:n]) | (y[:n] != y1[:n])))
        assert not n or ((x[:n] != x1[:n]) | (y[:n] != y1[:n])).all()      # the live rays are a prefix
    return np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)


def hit_cells(world, sensor_xy, resolution, height_min, height_max, max_range):
    """grid_cell_key (csrc/occupancy.h) on every world row with the sensor at sensor_xy: the (x, y) cells of the
    rows that mark one, (n, 2) int64 in row order.  The same IEEE operations, elementwise."""
    w = np.asarray(world, dtype=np.float64).reshape(-1, 3)
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    with np.errstate(all="ignore"):
        dx, dy = x - sensor_xy[0], y - sensor_xy[1]
        r = np.sqrt(dx * dx + dy * dy)
        cx, cy = np.floor(x / resolution), np.floor(y / resolution)
        ok = ~((z < height_min) | (z > height_max)) & ~((r > max_range) | (r < 0.5))
        ok &= (np.abs(cx) <= 2147483646.0) & (np.abs(cy) <= 2147483646.0)
    return np.stack([cx[ok], cy[ok]], axis=1).astype(np.int64)


def _unique_cells(cells):
    """(n, 2) int64 cells (|x|, |y| < 2^31) -> the distinct ones, sorted by x then y"""
    k = np.unique(cells[:, 0] * 2**32 + (cells[:, 1] + 2**31))     # one word per cell: a 1-D unique is much faster
    return np.stack([k >> 32, (k & (2**32 - 1)) - 2**31], axis=1)


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

    def raycast(self, poses, grid=None):
        """icpmi_map_raycast: every used frame's hits mark their cells occupied and carve the Bresenham line from the
        frame's sensor cell; 100 occupied, 0 carved and not occupied, -1 neither; bounds widened by 5 cells.  The limits
        the library refuses with ICPMI_ERR_ARG raise ValueError here."""
        g = grid_kwargs(grid)
        res = g["resolution"]
        if not (np.isfinite(res) and res > 0.0):
            raise ValueError("grid resolution must be finite and positive")
        with np.errstate(all="ignore"):
            Rd = np.ceil(np.float64(g["max_range"]) / res)
        if not Rd <= RAYCAST_MAX_R:
            raise ValueError("max_range / resolution must be at most %d cells" % RAYCAST_MAX_R)
        R = int(Rd) if Rd > 0 else 0
        last = min(len(self.clouds), len(poses))
        P = [np.asarray(poses[i], dtype=np.float64).reshape(4, 4) for i in range(last)]
        if not all(np.isfinite(T).all() for T in P):
            raise ValueError("a used pose has a non-finite entry")
        sensors = [(np.floor(T[0, 3] / res), np.floor(T[1, 3] / res)) for T in P]
        if any(abs(c) > 2147483646.0 - R - 6 for s in sensors for c in s):
            raise ValueError("a used frame's sensor cell is out of range")
        held = np.array([s for i, s in enumerate(sensors) if self.clouds[i].shape[0]], dtype=np.int64).reshape(-1, 2)
        if len(held):
            W, H = (int(v) + 2 * R + 3 for v in held.max(axis=0) - held.min(axis=0))
            if (W + 10) * (H + 10) > 2**31 - 1:
                raise ValueError("the used frames span more than 2^31 - 1 cells")
        occupied, carved = [], []
        for i in range(last):
            with np.errstate(all="ignore"):                             # non-finite rows mark nothing
                world = world_points(self.clouds[i], P[i])
            hits = _unique_cells(hit_cells(world, P[i][:2, 3], res, g["height_min"], g["height_max"], g["max_range"]))
            occupied.append(hits)
            s = sensors[i]
            carved.append(_unique_cells(bresenham_lockstep(int(s[0]), int(s[1]), hits[:, 0], hits[:, 1])))
        occupied = _unique_cells(np.concatenate(occupied)) if occupied else np.zeros((0, 2), dtype=np.int64)
        carved = _unique_cells(np.concatenate(carved)) if carved else np.zeros((0, 2), dtype=np.int64)
        both = np.concatenate([occupied, carved])
        if not len(both):
            return Raster(0, 0, 0, 0, res, 0, 0, np.zeros((0, 0), dtype=np.int8))
        lo, hi = both.min(axis=0) - 5, both.max(axis=0) + 5
        width, height = (int(v) for v in hi - lo + 1)
        data = np.full((height, width), UNKNOWN, dtype=np.int8)
        data[carved[:, 1] - lo[1], carved[:, 0] - lo[0]] = FREE
        data[occupied[:, 1] - lo[1], occupied[:, 0] - lo[0]] = OCCUPIED      # occupied wins
        return Raster(lo[0], lo[1], width, height, res, len(occupied), int(np.count_nonzero(data == FREE)), data)

    def raycast_counts(self, poses, grid=None):
        """icpmi_map_raycast_counts, normatively.  The frames (i < min(frames, len(poses))), poses, grid, hit cells,
        sensor cells and ray walk are raycast's.  For a used frame i, H_i is the set of its distinct hit cells and C_i
        the set of cells carved by any of its rays, minus H_i (within one scan occupied wins).  For a cell c,
        hits[c] = #{i : c in H_i} and misses[c] = #{i : c in C_i}: a frame adds at most 1 to each.  probability is -1
        where hits + misses == 0, else (200 hits + n) // (2 n) with n = hits + misses.  Bounds: tight over the cells
        with hits + misses > 0, widened by 5; nothing observed gives 0 x 0.  The limits the library refuses with
        ICPMI_ERR_ARG raise ValueError here: raycast's, and more than Counts.MAX_FRAMES used frames."""
        g = grid_kwargs(grid)
        res = g["resolution"]
        if not (np.isfinite(res) and res > 0.0):
            raise ValueError("grid resolution must be finite and positive")
        with np.errstate(all="ignore"):
            Rd = np.ceil(np.float64(g["max_range"]) / res)
        if not Rd <= RAYCAST_MAX_R:
            raise ValueError("max_range / resolution must be at most %d cells" % RAYCAST_MAX_R)
        R = int(Rd) if Rd > 0 else 0
        last = min(len(self.clouds), len(poses))
        if last > Counts.MAX_FRAMES:
            raise ValueError("more than %d frames would be used" % Counts.MAX_FRAMES)
        P = [np.asarray(poses[i], dtype=np.float64).reshape(4, 4) for i in range(last)]
        if not all(np.isfinite(T).all() for T in P):
            raise ValueError("a used pose has a non-finite entry")
        sensors = [(np.floor(T[0, 3] / res), np.floor(T[1, 3] / res)) for T in P]
        if any(abs(c) > 2147483646.0 - R - 6 for s in sensors for c in s):
            raise ValueError("a used frame's sensor cell is out of range")
        held = np.array([s for i, s in enumerate(sensors) if self.clouds[i].shape[0]], dtype=np.int64).reshape(-1, 2)
        if len(held):
            W, H = (int(v) + 2 * R + 3 for v in held.max(axis=0) - held.min(axis=0))
            if (W + 10) * (H + 10) > 2**31 - 1:
                raise ValueError("the used frames span more than 2^31 - 1 cells")
        key = lambda cells: cells[:, 0] * 2**32 + (cells[:, 1] + 2**31)     # noqa: E731  (_unique_cells' word per cell)
        hit_keys, miss_keys = [], []
        for i in range(last):
            with np.errstate(all="ignore"):                             # non-finite rows mark nothing
                world = world_points(self.clouds[i], P[i])
            H_i = _unique_cells(hit_cells(world, P[i][:2, 3], res, g["height_min"], g["height_max"], g["max_range"]))
            s = sensors[i]
            carved = _unique_cells(bresenham_lockstep(int(s[0]), int(s[1]), H_i[:, 0], H_i[:, 1]))
            hit_keys.append(key(H_i))
            miss_keys.append(np.setdiff1d(key(carved), key(H_i), assume_unique=True))   # C_i
        empty = np.zeros((0,), dtype=np.int64)
        hk, hn = np.unique(np.concatenate(hit_keys + [empty]), return_counts=True)      # a frame lists a cell once
        mk, mn = np.unique(np.concatenate(miss_keys + [empty]), return_counts=True)
        both = np.concatenate([hk, mk])
        if not len(both):
            z16 = np.zeros((0, 0), dtype=np.uint16)
            return Counts(0, 0, 0, 0, res, 0, 0, 0, 0, last, z16, z16.copy(), np.zeros((0, 0), dtype=np.int8))
        xy = lambda k: (k >> 32, (k & (2**32 - 1)) - 2**31)                 # noqa: E731
        bx, by = xy(both)
        lo = np.array([bx.min(), by.min()]) - 5
        width, height = int(bx.max()) + 5 - int(lo[0]) + 1, int(by.max()) + 5 - int(lo[1]) + 1
        hits, misses = np.zeros((height, width), dtype=np.uint16), np.zeros((height, width), dtype=np.uint16)
        x, y = xy(hk)
        hits[y - lo[1], x - lo[0]] = hn
        x, y = xy(mk)
        misses[y - lo[1], x - lo[0]] = mn
        return Counts(lo[0], lo[1], width, height, res, int(np.count_nonzero(hits | misses)), len(hk),
                      hits.max(), misses.max(), last, hits, misses, Counts.probability_of(hits, misses))


class MapRefLive(MapRef):
    """icpmi_map_live_update, normatively: the counts kept while frames arrive.  The host's decision is restated as it
    stands in the library: with used = min(frames, len(poses)), the update is incremental when the grid is bitwise
    the remembered one, used >= n_cast and the first n_cast poses are bitwise the remembered ones, and then only frames
    [n_cast, used) are cast; in every other case everything remembered is dropped and frames [0, used) are cast.  A
    frame's H_i and C_i (raycast_counts' definition) are added into two dictionaries, cell -> count, that persist; since
    the counts are sums over sets, live_counts() must equal raycast_counts(poses, grid) after every update, which
    tests/test_live_reference.py asserts.  An input raycast_counts refuses raises ValueError and changes nothing."""

    def __init__(self):
        super().__init__()
        self.live_clear()

    def live_clear(self):
        self._grid, self._cast, self._res = None, [], 0.0       # the grid's and each cast pose's bytes
        self._hits, self._misses = {}, {}                       # _unique_cells' word per cell -> count

    @staticmethod
    def _grid_bytes(g):
        return np.array([g["resolution"], g["height_min"], g["height_max"], g["max_range"]], dtype=np.float64).tobytes()

    def live_update(self, poses, grid=None):
        """-> (frames_cast, rebuilt), icpmi_live_info's"""
        g = grid_kwargs(grid)
        res = g["resolution"]
        if not (np.isfinite(res) and res > 0.0):
            raise ValueError("grid resolution must be finite and positive")
        with np.errstate(all="ignore"):
            Rd = np.ceil(np.float64(g["max_range"]) / res)
        if not Rd <= RAYCAST_MAX_R:
            raise ValueError("max_range / resolution must be at most %d cells" % RAYCAST_MAX_R)
        R = int(Rd) if Rd > 0 else 0
        used = min(len(self.clouds), len(poses))
        P = [np.ascontiguousarray(np.asarray(poses[i], dtype=np.float64).reshape(4, 4)) for i in range(used)]
        if not all(np.isfinite(T).all() for T in P):
            raise ValueError("a used pose has a non-finite entry")
        if used > Counts.MAX_FRAMES:
            raise ValueError("more than %d frames would be used" % Counts.MAX_FRAMES)
        sensors = [(np.floor(T[0, 3] / res), np.floor(T[1, 3] / res)) for T in P]
        if any(abs(c) > 2147483646.0 - R - 6 for s in sensors for c in s):
            raise ValueError("a used frame's sensor cell is out of range")
        held = np.array([s for i, s in enumerate(sensors) if self.clouds[i].shape[0]], dtype=np.int64).reshape(-1, 2)
        if len(held):
            W, H = (int(v) + 2 * R + 3 for v in held.max(axis=0) - held.min(axis=0))
            if (W + 10) * (H + 10) > 2**31 - 1:
                raise ValueError("the used frames span more than 2^31 - 1 cells")
        # the decision
        n_cast = len(self._cast)
        incremental = (self._grid == self._grid_bytes(g) and used >= n_cast
                       and all(P[i].tobytes() == self._cast[i] for i in range(n_cast)))
        rebuilt = int(not incremental and n_cast > 0)
        if not incremental:
            self.live_clear()
            n_cast = 0
        self._grid, self._res = self._grid_bytes(g), res
        for i in range(n_cast, used):
            with np.errstate(all="ignore"):
                world = world_points(self.clouds[i], P[i])
            H_i = _unique_cells(hit_cells(world, P[i][:2, 3], res, g["height_min"], g["height_max"], g["max_range"]))
            s = sensors[i]
            carved = _unique_cells(bresenham_lockstep(int(s[0]), int(s[1]), H_i[:, 0], H_i[:, 1]))
            hk = H_i[:, 0] * 2**32 + (H_i[:, 1] + 2**31)
            ck = carved[:, 0] * 2**32 + (carved[:, 1] + 2**31)
            for k in hk.tolist():
                self._hits[k] = self._hits.get(k, 0) + 1
            for k in np.setdiff1d(ck, hk, assume_unique=True).tolist():     # C_i
                self._misses[k] = self._misses.get(k, 0) + 1
            self._cast.append(P[i].tobytes())
        return used - n_cast, rebuilt

    def live_counts(self):
        """the Counts of the frames cast so far"""
        last = len(self._cast)
        keys = np.array(sorted(set(self._hits) | set(self._misses)), dtype=np.int64)
        if not len(keys):
            z16 = np.zeros((0, 0), dtype=np.uint16)
            return Counts(0, 0, 0, 0, self._res, 0, 0, 0, 0, last, z16, z16.copy(), np.zeros((0, 0), dtype=np.int8))
        x, y = keys >> 32, (keys & (2**32 - 1)) - 2**31
        lo = np.array([x.min(), y.min()]) - 5
        width, height = int(x.max()) + 5 - int(lo[0]) + 1, int(y.max()) + 5 - int(lo[1]) + 1
        hits, misses = np.zeros((height, width), dtype=np.uint16), np.zeros((height, width), dtype=np.uint16)
        hits[y - lo[1], x - lo[0]] = [self._hits.get(k, 0) for k in keys.tolist()]
        misses[y - lo[1], x - lo[0]] = [self._misses.get(k, 0) for k in keys.tolist()]
        return Counts(lo[0], lo[1], width, height, self._res, len(keys), len(self._hits), hits.max(), misses.max(), last,
                      hits, misses, Counts.probability_of(hits, misses))
