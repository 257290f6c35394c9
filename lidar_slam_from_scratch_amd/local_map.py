"""The sliding voxel map of scan-to-local-map odometry through the C ABI (icpmi_local_map; csrc/local_map.h): the recent
scans in one frame, at most one point per voxel, kept on the device as a registration target.  Not in the reference node,
which registers each scan against the one before it (slam_viz/src/ros/slam_node.cpp:132-138).  scripts/local_map_ref.py
restates the table and the driver (odometry.run_odometry_local_map) on the CPU, byte for byte."""
import ctypes as C
import weakref

import numpy as np

from . import capi


class LocalMapConfig:
    """voxel_size and max_range in metres, capacity in rows (64 bytes of device memory each).  max_range must cover the
    sensor's range: a scan whose far rows have no counterpart in the map loses the track."""

    def __init__(self, voxel_size=0.5, max_range=100.0, capacity=1 << 20):
        self.voxel_size, self.max_range, self.capacity = float(voxel_size), float(max_range), int(capacity)

    def to_c(self):
        c = capi.LocalMapConfig()
        c.voxel_size, c.max_range, c.capacity = self.voxel_size, self.max_range, self.capacity
        return c


def _pose(pose):
    return np.ascontiguousarray(pose, dtype=np.float64).reshape(16)


class LocalMap:
    def __init__(self, ctx, config=None):
        self._lib = capi.load_library()
        self.ctx = ctx
        self.config = config if config is not None else LocalMapConfig()
        c = self.config.to_c()
        h = C.c_void_p()
        ctx._check(self._lib.icpmi_local_map_create(ctx._h, C.byref(c), C.byref(h)))
        self._h = h
        if not hasattr(ctx, "_local_maps"):
            ctx._local_maps = weakref.WeakSet()
        ctx._local_maps.add(self)      # Context.close() destroys the handle first

    def close(self):
        if getattr(self, "_h", None):
            self._lib.icpmi_local_map_destroy(self._h)
            self._h = None

    __del__ = close

    def clear(self):
        self.ctx._check(self._lib.icpmi_local_map_clear(self._h))

    def add(self, scan, pose):
        """evict, insert, merge (icpmi_local_map_add) with the scan in host memory -> capi.LocalMapInfo"""
        pts = capi._f64(scan) if len(scan) else np.zeros((0, 3))
        T, info = _pose(pose), capi.LocalMapInfo()
        self.ctx._check(self._lib.icpmi_local_map_add(self._h, capi._dp(pts), pts.shape[0], capi._dp(T), C.byref(info)))
        return info

    def add_device(self, ptr, n_rows, pose):
        T, info = _pose(pose), capi.LocalMapInfo()
        self.ctx._check(self._lib.icpmi_local_map_add_device(self._h, C.c_void_p(ptr), int(n_rows), capi._dp(T), C.byref(info)))
        return info

    def add_stream_frame(self, pose):
        """the filtered scan the context's last stream_push* left resident, device to device"""
        T, info = _pose(pose), capi.LocalMapInfo()
        self.ctx._check(self._lib.icpmi_local_map_add_stream_frame(self._h, capi._dp(T), C.byref(info)))
        return info

    def size(self):
        n = C.c_int64(0)
        self.ctx._check(self._lib.icpmi_local_map_size(self._h, C.byref(n)))
        return n.value

    def points(self):
        """-> (points rows x 3 fp64, keys rows uint64), sorted by key"""
        n = self.size()
        pts, keys = np.empty((n, 3)), np.empty(n, dtype=np.uint64)
        got = C.c_int64(0)
        self.ctx._check(self._lib.icpmi_local_map_points(self._h, capi._dp(pts), keys.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                                                         C.byref(got)))
        return pts, keys

    def register(self, scan, cfg):
        """icp_point_to_plane(scan, the table's points, cfg) -> (Result, error history); cfg.initial_transform is the
        guess in the map's frame, Result.transformation the scan's pose in it"""
        src = capi._f64(scan)
        cap = cfg.max_iterations + 1
        hist, res = np.zeros(max(cap, 1)), capi.Result()
        self.ctx._check(self._lib.icpmi_local_map_register(self._h, capi._dp(src), src.shape[0], C.byref(cfg), C.byref(res),
                                                           capi._dp(hist), cap))
        return res, hist[:res.history_len].copy()

    def register_device(self, ptr, n_rows, cfg):
        cap = cfg.max_iterations + 1
        hist, res = np.zeros(max(cap, 1)), capi.Result()
        self.ctx._check(self._lib.icpmi_local_map_register_device(self._h, C.c_void_p(ptr), int(n_rows), C.byref(cfg),
                                                                  C.byref(res), capi._dp(hist), cap))
        return res, hist[:res.history_len].copy()

    def register_robust(self, scan, cfg, rule):
        """register under robust row weights (rule: see capi.as_robust) -> (Result, error history, RobustInfo)"""
        src = capi._f64(scan)
        cap = cfg.max_iterations + 1
        hist, res, info, r = np.zeros(max(cap, 1)), capi.Result(), capi.RobustInfo(), capi.as_robust(rule)
        self.ctx._check(self._lib.icpmi_local_map_register_robust(self._h, capi._dp(src), src.shape[0], C.byref(cfg), C.byref(r),
                                                                  C.byref(res), C.byref(info), capi._dp(hist), cap))
        return res, hist[:res.history_len].copy(), info

    def register_robust_device(self, ptr, n_rows, cfg, rule):
        cap = cfg.max_iterations + 1
        hist, res, info, r = np.zeros(max(cap, 1)), capi.Result(), capi.RobustInfo(), capi.as_robust(rule)
        self.ctx._check(self._lib.icpmi_local_map_register_robust_device(self._h, C.c_void_p(ptr), int(n_rows), C.byref(cfg),
                                                                         C.byref(r), C.byref(res), C.byref(info),
                                                                         capi._dp(hist), cap))
        return res, hist[:res.history_len].copy(), info
