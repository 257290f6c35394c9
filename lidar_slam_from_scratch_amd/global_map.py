"""The node's global map through the C ABI (icpmi_map): SlamNode keeps every filtered scan (downsampled_clouds_,
slam_viz/src/ros/slam_node.cpp:71,123) and, with the optimised poses, rebuilds the recent clouds after each successful
optimize (rebuild_recent_clouds, :187-194), and at the end the global map, the occupancy set (build_final_global_map,
rebuild_occupancy_grid, :196-209, :223-229) and the map it publishes (publish_global_map, :235-238).  Here the scans
stay in device memory (csrc/global_map.h); scripts/map_ref.py restates the same interface on the CPU."""
import ctypes as C
import weakref

import numpy as np

from . import capi

MAX_RECENT_CLOUDS = 20   # slam_node.hpp:169


def _poses(poses):
    P = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4))
    return P, (capi._dp(P) if P.shape[0] else None)


class OccupancyRaster:
    """icpmi_map_raster's result: the info fields, and data[y - min_y, x - min_x] as (height, width) int8:
    100 occupied, 0 free, -1 unknown"""

    def __init__(self, info, data):
        self.min_x, self.min_y, self.width, self.height = info.min_x, info.min_y, info.width, info.height
        self.resolution, self.n_occupied, self.n_free = info.resolution, info.n_occupied, info.n_free
        self.data = data


class OccupancyCounts:
    """icpmi_map_counts' result: the info fields, and hits, misses (uint16) and probability (int8: -1 unobserved, else
    100 hits / (hits + misses) rounded half up), each [y - min_y, x - min_x] as (height, width)"""

    def __init__(self, info, hits, misses, probability):
        self.min_x, self.min_y, self.width, self.height = info.min_x, info.min_y, info.width, info.height
        self.resolution, self.n_observed, self.n_hit_cells = info.resolution, info.n_observed, info.n_hit_cells
        self.max_hits, self.max_misses, self.frames_used = info.max_hits, info.max_misses, info.frames_used
        self.hits, self.misses, self.probability = hits, misses, probability


class GlobalMap:
    def __init__(self, ctx):
        self._lib = capi.load_library()
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(self._lib.icpmi_map_create(ctx._h, C.byref(h)))
        self._h = h
        self._rows = []                # rows per frame, in order
        if not hasattr(ctx, "_maps"):
            ctx._maps = weakref.WeakSet()
        ctx._maps.add(self)            # Context.close() destroys the map first

    def close(self):
        if getattr(self, "_h", None):
            for d in list(getattr(self, "_loops", ())):   # loop_closure.StoreLoopClosureDetector handles go first
                d.close()
            self._lib.icpmi_map_destroy(self._h)
            self._h = None

    __del__ = close

    def add_frame(self, cloud):
        """downsampled_clouds_.push_back(curr) (slam_node.cpp:71,123) with the rows in host memory"""
        pts = capi._f64(cloud) if len(cloud) else np.zeros((0, 3))
        self.ctx._check(self._lib.icpmi_map_add_frame(self._h, capi._dp(pts), pts.shape[0]))
        self._rows.append(pts.shape[0])

    def add_frame_device(self, ptr, n_rows):
        self.ctx._check(self._lib.icpmi_map_add_frame_device(self._h, C.c_void_p(ptr), int(n_rows)))
        self._rows.append(int(n_rows))

    def add_stream_frame(self):
        """the filtered scan the context's last stream_push* left resident, device to device"""
        before = self.size()[1]
        self.ctx._check(self._lib.icpmi_map_add_stream_frame(self._h))
        self._rows.append(self.size()[1] - before)

    def size(self):
        """(frames, rows)"""
        f, n = C.c_int64(0), C.c_int64(0)
        self.ctx._check(self._lib.icpmi_map_size(self._h, C.byref(f), C.byref(n)))
        return f.value, n.value

    def world(self, poses, first=0):
        """world points of frames [first, min(frames, len(poses))), frame then row order: N x 3"""
        P, pp = _poses(poses)
        n = C.c_int64(0)
        self.ctx._check(self._lib.icpmi_map_world(self._h, pp, P.shape[0], int(first), None, 0, C.byref(n)))
        out = np.empty((n.value, 3))
        if n.value:
            self.ctx._check(self._lib.icpmi_map_world(self._h, pp, P.shape[0], int(first), capi._dp(out), n.value,
                                                      C.byref(n)))
        return out

    def recent_clouds(self, poses, max_recent=MAX_RECENT_CLOUDS):
        """rebuild_recent_clouds (slam_node.cpp:187-194): one world cloud per frame, for the last max_recent frames"""
        frames = len(self._rows)
        first = frames - max_recent if frames > max_recent else 0
        last = min(frames, len(poses))
        w = self.world(poses, first)
        bounds = np.cumsum([0] + self._rows[first:last])
        return [w[bounds[i]:bounds[i + 1]] for i in range(max(0, last - first))]

    def finish(self, poses, grid=None, voxel=1.0):
        """build_final_global_map -> rebuild_occupancy_grid (slam_node.cpp:196-209, :223-229) into the context's cell
        set, and voxel_downsample(global map, voxel) (:235-238).  grid None: the default OccupancyGridConfig.
        Returns (cells: (n, 2) int32 sorted by x then y, published map: M x 3)."""
        P, pp = _poses(poses)
        g = grid if grid is not None else self.ctx.make_grid_config()
        rows = int(sum(self._rows[:min(len(self._rows), P.shape[0])]))
        out = np.empty((max(rows, 1), 3))
        nm, nc = C.c_int64(0), C.c_int64(0)
        self.ctx._check(self._lib.icpmi_map_finish(self._h, pp, P.shape[0], C.byref(g), float(voxel), capi._dp(out),
                                                   rows, C.byref(nm), C.byref(nc)))
        return self.ctx.occupancy_cells(), out[:nm.value].copy()

    def raster(self):
        """the last successful raycast's raster (0 x 0 before the first)"""
        info = capi.RasterInfo()
        self.ctx._check(self._lib.icpmi_map_raster(self._h, None, 0, C.byref(info)))
        data = np.empty((info.height, info.width), dtype=np.int8)
        if data.size:
            self.ctx._check(self._lib.icpmi_map_raster(self._h, data.ctypes.data_as(C.POINTER(C.c_int8)), data.size,
                                                       C.byref(info)))
        return OccupancyRaster(info, data)

    def raycast(self, poses, grid=None):
        """The kept scans ray-cast into a free / occupied / unknown raster (icpmi_map_raycast): every hit marks its cell
        occupied and carves the Bresenham line from its frame's sensor cell to it.  grid None: the default
        OccupancyGridConfig.  The context's cell set is not touched.  Returns an OccupancyRaster."""
        P, pp = _poses(poses)
        g = grid if grid is not None else self.ctx.make_grid_config()
        self.ctx._check(self._lib.icpmi_map_raycast(self._h, pp, P.shape[0], C.byref(g), None))
        return self.raster()

    def counts(self):
        """the last successful raycast_counts' arrays (0 x 0 before the first)"""
        info = capi.CountsInfo()
        self.ctx._check(self._lib.icpmi_map_counts(self._h, None, None, None, 0, C.byref(info)))
        shape = (info.height, info.width)
        hits, misses = np.empty(shape, dtype=np.uint16), np.empty(shape, dtype=np.uint16)
        probability = np.empty(shape, dtype=np.int8)
        if hits.size:
            u16 = C.POINTER(C.c_uint16)
            self.ctx._check(self._lib.icpmi_map_counts(self._h, hits.ctypes.data_as(u16), misses.ctypes.data_as(u16),
                                                       probability.ctypes.data_as(C.POINTER(C.c_int8)), hits.size,
                                                       C.byref(info)))
        return OccupancyCounts(info, hits, misses, probability)

    def raycast_counts(self, poses, grid=None):
        """The kept scans ray-cast into per-cell hit and miss counts (icpmi_map_raycast_counts): a used frame adds 1 to
        the hits of each of its distinct hit cells and 1 to the misses of every other cell its rays carve.  grid None:
        the default OccupancyGridConfig.  Neither the context's cell set nor raster() is touched.  Returns an
        OccupancyCounts."""
        P, pp = _poses(poses)
        g = grid if grid is not None else self.ctx.make_grid_config()
        self.ctx._check(self._lib.icpmi_map_raycast_counts(self._h, pp, P.shape[0], C.byref(g), None))
        return self.counts()

    def live_update(self, poses, grid=None):
        """The counts kept while the node drives (icpmi_map_live_update): afterwards the handle's live counts are byte
        for byte what raycast_counts(poses, grid) would build, but only the frames not yet cast are cast, unless a pose
        already cast or the grid has changed.  grid None: the default OccupancyGridConfig.  Neither counts(), raster()
        nor the context's cell set is touched.  Returns the capi.LiveInfo."""
        P, pp = _poses(poses)
        g = grid if grid is not None else self.ctx.make_grid_config()
        info = capi.LiveInfo()
        self.ctx._check(self._lib.icpmi_map_live_update(self._h, pp, P.shape[0], C.byref(g), C.byref(info)))
        return info

    def live_counts(self):
        """(OccupancyCounts, capi.LiveInfo) of the last successful live_update (0 x 0 before the first)"""
        info = capi.LiveInfo()
        self.ctx._check(self._lib.icpmi_map_live_counts(self._h, None, None, None, 0, C.byref(info)))
        shape = (info.counts.height, info.counts.width)
        hits, misses = np.empty(shape, dtype=np.uint16), np.empty(shape, dtype=np.uint16)
        probability = np.empty(shape, dtype=np.int8)
        if hits.size:
            u16 = C.POINTER(C.c_uint16)
            self.ctx._check(self._lib.icpmi_map_live_counts(self._h, hits.ctypes.data_as(u16), misses.ctypes.data_as(u16),
                                                            probability.ctypes.data_as(C.POINTER(C.c_int8)), hits.size,
                                                            C.byref(info)))
        return OccupancyCounts(info.counts, hits, misses, probability), info

    def live_clear(self):
        """forget the frames cast so far: the next live_update casts every used frame again"""
        self.ctx._check(self._lib.icpmi_map_live_clear(self._h))

    def set_ground(self, ground):
        """icpmi_map_set_ground: with a ground.GroundConfig (or capi.GroundConfig), finish's cell set, raycast,
        raycast_counts and live_update take as a frame's hits its OBSTACLE rows instead of the grid's world-z band;
        None turns it off.  Either way the next live_update rebuilds."""
        g = ground.to_c() if hasattr(ground, "to_c") else ground
        self.ctx._check(self._lib.icpmi_map_set_ground(self._h, C.byref(g) if g is not None else None))

    def ground_labels(self, frame):
        """one frame's cached labels (uint8 per row: capi.GROUND_OBSTACLE, GROUND_GROUND, GROUND_IGNORED), formed first if
        need be; needs a ground config"""
        n = C.c_int64(0)
        self.ctx._check(self._lib.icpmi_map_ground_labels(self._h, int(frame), None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.uint8)
        self.ctx._check(self._lib.icpmi_map_ground_labels(self._h, int(frame), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                          n.value, C.byref(n)))
        return out

    # ---- the static map (icpmi_map_world_static / icpmi_map_finish_static; csrc/static_map.h) ----

    def world_static(self, poses, grid=None, rule=None, first=0):
        """world() without the rows the counts outvote: the world points of the rows of frames [first, min(frames,
        len(poses))) that the rule keeps, frame then row order, each bit for bit world()'s.  The live counts are brought
        up to date first, as by live_update(poses, grid), and every used row is labelled against them (static_labels).
        grid None: the default OccupancyGridConfig -- whose band holds no car roof with the sensor at z = 0: see
        include/icp_mi355x.h.  rule: a capi.StaticRule or (min_probability, min_observations); None: the defaults.
        Returns (N x 3, capi.StaticInfo)."""
        P, pp = _poses(poses)
        g = grid if grid is not None else self.ctx.make_grid_config()
        r = capi.as_static_rule(rule) if rule is not None else capi.StaticRule()
        n, info = C.c_int64(0), capi.StaticInfo()
        last = min(len(self._rows), P.shape[0])
        cap = int(sum(self._rows[min(max(int(first), 0), last):last]))      # one call: info.live is that call's update
        out = np.empty((max(cap, 1), 3))
        self.ctx._check(self._lib.icpmi_map_world_static(self._h, pp, P.shape[0], C.byref(g), C.byref(r), int(first),
                                                         capi._dp(out), cap, C.byref(n), C.byref(info)))
        return out[:n.value].copy(), info

    def recent_clouds_static(self, poses, grid=None, rule=None, max_recent=MAX_RECENT_CLOUDS):
        """recent_clouds() without the dropped rows: one world cloud per frame, for the last max_recent frames"""
        frames = len(self._rows)
        first = frames - max_recent if frames > max_recent else 0
        last = min(frames, len(poses))
        w, _ = self.world_static(poses, grid, rule, first)
        kept = [int(np.count_nonzero(self.static_labels(i) != capi.STATIC_DROPPED)) for i in range(first, last)]
        bounds = np.cumsum([0] + kept)
        return [w[bounds[i]:bounds[i + 1]] for i in range(max(0, last - first))]

    def finish_static(self, poses, grid=None, rule=None, voxel=1.0):
        """finish()'s published map over the kept rows of all used frames: voxel_downsample(kept world rows, voxel).
        The context's cell set is not touched.  Returns (published map: M x 3, capi.StaticInfo)."""
        P, pp = _poses(poses)
        g = grid if grid is not None else self.ctx.make_grid_config()
        r = capi.as_static_rule(rule) if rule is not None else capi.StaticRule()
        rows = int(sum(self._rows[:min(len(self._rows), P.shape[0])]))
        out = np.empty((max(rows, 1), 3))
        nm, info = C.c_int64(0), capi.StaticInfo()
        self.ctx._check(self._lib.icpmi_map_finish_static(self._h, pp, P.shape[0], C.byref(g), C.byref(r), float(voxel),
                                                          capi._dp(out), rows, C.byref(nm), C.byref(info)))
        return out[:nm.value].copy(), info

    def static_labels(self, frame):
        """one frame's labels (uint8 per row: capi.STATIC_QUIET, STATIC_VOTES, STATIC_DROPPED) as the last world_static or
        finish_static left them; an error before any, or for a frame that call did not use"""
        n = C.c_int64(0)
        self.ctx._check(self._lib.icpmi_map_static_labels(self._h, int(frame), None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.uint8)
        self.ctx._check(self._lib.icpmi_map_static_labels(self._h, int(frame), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                          n.value, C.byref(n)))
        return out
