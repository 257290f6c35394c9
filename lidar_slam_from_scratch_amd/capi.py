"""ctypes binding of include/icp_mi355x.h (the C ABI of libicp_mi355x.so).

The library is the product; there is deliberately no Python or CPU fallback here:
if the shared object is missing or no gfx950 device is visible, calls raise.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

OK = 0
ERR_NULL, ERR_EMPTY_SOURCE, ERR_EMPTY_TARGET, ERR_CAPACITY = -1, -2, -3, -4
ERR_HIP, ERR_RCCL, ERR_ARG, ERR_NO_DEVICE = -5, -6, -7, -8
SEARCH_AUTO, SEARCH_EXACT_F64, SEARCH_MFMA_BF16, SEARCH_MFMA_PRUNED = 0, 1, 2, 3
DEBUG_NO_IDX = 1   # icpmi_debug_loop_rows: the last pass's matches were not kept (small-cloud kernel)
UNIQUE_ID_BYTES = 128

EXPORTS = [
    "icpmi_version", "icpmi_options_default", "icpmi_config_default", "icpmi_create",
    "icpmi_destroy", "icpmi_last_error", "icpmi_align", "icpmi_align_device", "icpmi_align_batch",
    "icpmi_nearest_batch", "icpmi_k_nearest", "icpmi_estimate_normals", "icpmi_solve_point_to_plane",
    "icpmi_transform_points", "icpmi_comm_unique_id", "icpmi_comm_init", "icpmi_comm_finalize",
    "icpmi_comm_init_callbacks", "icpmi_comm_info", "icpmi_voxel_downsample", "icpmi_voxel_downsample_device",
    "icpmi_scan_context", "icpmi_scan_context_distances", "icpmi_load_cloud", "icpmi_load_cloud_device",
    "icpmi_upload_points_f32", "icpmi_discover_frames", "icpmi_estimate_normals_rows",
    "icpmi_stream_push", "icpmi_stream_push_host", "icpmi_stream_push_file", "icpmi_stream_prefetch_file", "icpmi_stream_reset",
    "icpmi_grid_config_default", "icpmi_occupancy_update", "icpmi_occupancy_update_device", "icpmi_occupancy_cells",
    "icpmi_occupancy_clear", "icpmi_stream_map_update", "icpmi_stream_current_scan",
    "icpmi_reset_profile", "icpmi_get_profile",
    "icpmi_pose_graph_config_default", "icpmi_pose_graph_create", "icpmi_pose_graph_destroy",
    "icpmi_pose_graph_add_prior", "icpmi_pose_graph_add_odometry", "icpmi_pose_graph_add_loop_closure",
    "icpmi_pose_graph_optimize", "icpmi_pose_graph_pose", "icpmi_pose_graph_poses", "icpmi_pose_graph_size",
    "icpmi_map_create", "icpmi_map_destroy", "icpmi_map_add_frame", "icpmi_map_add_frame_device",
    "icpmi_map_add_stream_frame", "icpmi_map_size", "icpmi_map_world", "icpmi_map_finish",
    "icpmi_map_raycast", "icpmi_map_raster", "icpmi_map_raycast_counts", "icpmi_map_counts",
    "icpmi_map_live_update", "icpmi_map_live_counts", "icpmi_map_live_clear",
    "icpmi_loop_config_default", "icpmi_loop_create", "icpmi_loop_destroy", "icpmi_loop_add_frame", "icpmi_loop_detect",
    "icpmi_loop_descriptor", "icpmi_loop_size", "icpmi_loop_clear",
    "icpmi_scan_context_distances_shift", "icpmi_sc_shift_transform", "icpmi_loop_set_yaw_guess", "icpmi_loop_last_shifts",
    "icpmi_align_gated", "icpmi_align_gated_device", "icpmi_align_gated_batch", "icpmi_loop_set_gate", "icpmi_loop_last_pairs",
    "icpmi_ground_config_default", "icpmi_ground_segment", "icpmi_ground_segment_device", "icpmi_map_set_ground",
    "icpmi_map_ground_labels",
    "icpmi_align_robust", "icpmi_align_robust_device", "icpmi_align_robust_batch", "icpmi_loop_set_robust",
    "icpmi_loop_last_weights", "icpmi_stream_set_robust", "icpmi_stream_last_robust",
    "icpmi_local_map_config_default", "icpmi_local_map_create", "icpmi_local_map_destroy", "icpmi_local_map_clear",
    "icpmi_local_map_add", "icpmi_local_map_add_device", "icpmi_local_map_add_stream_frame", "icpmi_local_map_size",
    "icpmi_local_map_points", "icpmi_local_map_register", "icpmi_local_map_register_device",
    "icpmi_local_map_register_robust", "icpmi_local_map_register_robust_device",
    "icpmi_pose_graph_set_loop_loss", "icpmi_pose_graph_loop_loss", "icpmi_pose_graph_loop_weights",
    "icpmi_pose_graph_add_odometry_information", "icpmi_pose_graph_add_loop_closure_information",
    "icpmi_pose_graph_marginals", "icpmi_pose_graph_relative_covariance", "icpmi_pose_graph_closure_distance",
    "icpmi_information_from_icp", "icpmi_last_normal_matrix", "icpmi_loop_set_information", "icpmi_loop_last_information",
    "icpmi_deskew_config_default", "icpmi_deskew", "icpmi_deskew_device", "icpmi_deskew_twist", "icpmi_stream_set_deskew",
    "icpmi_align_gicp", "icpmi_align_gicp_device", "icpmi_align_gicp_batch", "icpmi_loop_set_gicp",
    "icpmi_map_world_static", "icpmi_map_finish_static", "icpmi_map_static_labels",
]


class Options(C.Structure):
    _fields_ = [("device", C.c_int32), ("normal_k", C.c_int32), ("search", C.c_int32),
                ("profile", C.c_int32)]


class Config(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("reserved", C.c_int32),
                ("tolerance", C.c_double), ("min_error", C.c_double),
                ("initial_transform", C.c_double * 16)]


class Result(C.Structure):
    _fields_ = [("transformation", C.c_double * 16), ("converged", C.c_int32),
                ("num_iterations", C.c_int32), ("final_error", C.c_double),
                ("history_len", C.c_int32), ("loop_iterations", C.c_int32)]


class Gate(C.Structure):
    """icpmi_gate: the correspondence-distance gate of align_gated*"""
    _fields_ = [("max_distance", C.c_double), ("reserved", C.c_int32 * 2)]


class GateInfo(C.Structure):
    """icpmi_gate_info: rows kept by the pass that produced final_error, of `rows`"""
    _fields_ = [("pairs", C.c_int64), ("rows", C.c_int64)]


ROBUST_HUBER, ROBUST_GEMAN_MCCLURE = 1, 2   # ICPMI_ROBUST_*


class Robust(C.Structure):
    """icpmi_robust: the row weights of align_robust* (kind ROBUST_*, scale in metres of point-to-plane residual) and
    their optional correspondence-distance gate (max_distance; 0: none)"""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("scale", C.c_double), ("max_distance", C.c_double)]


class RobustInfo(C.Structure):
    """icpmi_robust_info: weight sum and kept rows of the pass that produced final_error, of `rows`"""
    _fields_ = [("weight_sum", C.c_double), ("pairs", C.c_int64), ("rows", C.c_int64)]


def as_robust(rule):
    """a Robust, or (kind, scale) or (kind, scale, max_distance) -> Robust"""
    if isinstance(rule, Robust):
        return rule
    r = Robust()
    r.kind, r.scale = int(rule[0]), float(rule[1])
    r.max_distance = float(rule[2]) if len(rule) > 2 else 0.0
    return r


GICP_EPSILON_DEFAULT = 1e-3                 # ICPMI_GICP_EPSILON_DEFAULT
GICP_FORM_SMALL = 1                         # ICPMI_GICP_FORM_SMALL, bit 0 of Gicp.reserved


class Gicp(C.Structure):
    """icpmi_gicp: the rule of align_gicp* (plane-to-plane ICP): epsilon, the covariance along a row's normal relative to
    1 in its plane (1: point-to-point), the optional correspondence-distance gate (max_distance; 0: none) and the form
    (reserved: GICP_FORM_SMALL -- one kernel per pass at the small-cloud kernel's sizes -- or 0, the general path)"""
    _fields_ = [("epsilon", C.c_double), ("max_distance", C.c_double), ("reserved", C.c_int64)]


class GicpInfo(C.Structure):
    """icpmi_gicp_info: rows kept by the pass that produced final_error, of `rows`"""
    _fields_ = [("pairs", C.c_int64), ("rows", C.c_int64)]


def as_gicp(rule):
    """a Gicp, or (epsilon[, max_distance[, small]]) -> Gicp (small: the small form where the sizes allow it,
    GICP_FORM_SMALL; default: the general path)"""
    if isinstance(rule, Gicp):
        return rule
    g = Gicp()
    g.epsilon = float(rule[0])
    g.max_distance = float(rule[1]) if len(rule) > 1 else 0.0
    g.reserved = GICP_FORM_SMALL if len(rule) > 2 and rule[2] else 0
    return g


class NormalMatrix(C.Structure):
    """icpmi_normal_matrix: the normal equations of the pass that produced final_error"""
    _fields_ = [("JtJ", C.c_double * 36), ("Jtb", C.c_double * 6), ("sum_sq", C.c_double), ("weight", C.c_double),
                ("pairs", C.c_int64), ("T", C.c_double * 16)]


class LoopConfig(C.Structure):
    _fields_ = [("frame_gap", C.c_int32), ("max_candidates", C.c_int32),
                ("sc_distance_threshold", C.c_double), ("icp_fitness_threshold", C.c_double)]


class LoopResult(C.Structure):
    _fields_ = [("query_frame", C.c_int32), ("match_frame", C.c_int32), ("transform", C.c_double * 16),
                ("scan_context_distance", C.c_double), ("icp_fitness", C.c_double)]


class Profile(C.Structure):
    _fields_ = [("nn_ms", C.c_double), ("nn_launches", C.c_int64),
                ("coarse_ms", C.c_double), ("coarse_launches", C.c_int64),
                ("reduce_ms", C.c_double), ("reduce_launches", C.c_int64),
                ("transform_ms", C.c_double), ("transform_launches", C.c_int64),
                ("normals_ms", C.c_double), ("normals_launches", C.c_int64),
                ("total_ms", C.c_double), ("calls", C.c_int64), ("loop_ms", C.c_double),
                ("setup_ms", C.c_double),
                ("nn_pairs", C.c_double), ("nn_recheck_queries", C.c_int64),
                ("nn_fallback_queries", C.c_int64), ("knn_fallback_rows", C.c_int64),
                ("nn_coarse_blocks", C.c_int64), ("nn_pruned_blocks", C.c_int64), ("small_launches", C.c_int64),
                ("bounded_launches", C.c_int64),
                ("nn_group_pairs", C.c_int64),
                ("nn_group_pairs_run", C.c_int64),
                ("exchange_ms", C.c_double), ("exchange_launches", C.c_int64), ("coarse_minima_bytes", C.c_int64),
                ("nn_rows_listed", C.c_int64), ("nn_coarse_skipped", C.c_int64),
                ("knn_culled_launches", C.c_int64), ("nn_rows_certified", C.c_int64),
                ("nn_lean_passes", C.c_int64), ("nn_full_culled_passes", C.c_int64),
                ("nn_solo_passes", C.c_int64), ("nn_solo_fallback_rows", C.c_int64)]


MAX_RANKS_INFO = 64
MAX_BATCH = 8   # ICPMI_MAX_BATCH


class CommInfo(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n_ranks", C.c_int32), ("rank", C.c_int32), ("reserved", C.c_int32),
                ("device", C.c_int32 * MAX_RANKS_INFO), ("pci_bus_id", (C.c_char * 16) * MAX_RANKS_INFO)]


class StreamInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("reserved", C.c_int32), ("n_filtered", C.c_int64), ("n_target", C.c_int64)]


STREAM_REGISTERED, STREAM_FIRST_FRAME, STREAM_TOO_FEW_POINTS = 0, 1, 2


class GridConfig(C.Structure):
    """OccupancyGridConfig (slam_node.hpp:35-40)"""
    _fields_ = [("resolution", C.c_double), ("height_min", C.c_double), ("height_max", C.c_double), ("max_range", C.c_double)]


RAYCAST_MAX_R, RAYCAST_LDS_MAX_R = 4096, 559   # ICPMI_RAYCAST_MAX_R, ICPMI_RAYCAST_LDS_MAX_R


class RasterInfo(C.Structure):
    """icpmi_raster_info"""
    _fields_ = [("min_x", C.c_int32), ("min_y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("resolution", C.c_double), ("n_occupied", C.c_int64), ("n_free", C.c_int64)]


RAYCOUNT_MAX_FRAMES, RAYCOUNT_LDS_MAX_R = 65535, 392   # ICPMI_RAYCOUNT_MAX_FRAMES, ICPMI_RAYCOUNT_LDS_MAX_R


class CountsInfo(C.Structure):
    """icpmi_counts_info"""
    _fields_ = [("min_x", C.c_int32), ("min_y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("resolution", C.c_double), ("n_observed", C.c_int64), ("n_hit_cells", C.c_int64),
                ("max_hits", C.c_int32), ("max_misses", C.c_int32), ("frames_used", C.c_int32), ("pad", C.c_int32)]


LIVE_CARVE_GROUPS, LIVE_CARVE_ROWS = 16, 1024   # csrc/live_counts.h's kLiveGroups and kLiveGroupRows: a new frame's rows
#                                                 are shared among min(16, ceil(rows / 1024)) workgroups


class LiveInfo(C.Structure):
    """icpmi_live_info"""
    _fields_ = [("counts", CountsInfo), ("frames_cast", C.c_int64), ("rebuilt", C.c_int32), ("moved", C.c_int32),
                ("plane_x0", C.c_int32), ("plane_y0", C.c_int32), ("plane_w", C.c_int32), ("plane_h", C.c_int32)]


STATIC_MIN_PROBABILITY_DEFAULT, STATIC_MIN_OBSERVATIONS_DEFAULT = 50, 3   # ICPMI_STATIC_*_DEFAULT
STATIC_QUIET, STATIC_VOTES, STATIC_DROPPED = 0, 1, 2      # a row's label: kept and does not vote, kept and votes, dropped


class StaticRule(C.Structure):
    """icpmi_static_rule: a voting row is dropped if its cell was observed by at least min_observations frames and its
    probability is below min_probability (0 drops nothing)"""
    _fields_ = [("min_probability", C.c_int32), ("min_observations", C.c_int32), ("reserved", C.c_int64)]

    def __init__(self, min_probability=STATIC_MIN_PROBABILITY_DEFAULT, min_observations=STATIC_MIN_OBSERVATIONS_DEFAULT, reserved=0):
        super().__init__(int(min_probability), int(min_observations), int(reserved))


class StaticInfo(C.Structure):
    """icpmi_static_info: over the used frames, their rows, those that vote, those dropped and rows - dropped; and what
    the live update at the head of the call reports"""
    _fields_ = [("rows", C.c_int64), ("voting", C.c_int64), ("dropped", C.c_int64), ("kept", C.c_int64), ("live", LiveInfo)]


def as_static_rule(rule):
    """a StaticRule, or (min_probability, min_observations) -> StaticRule"""
    if isinstance(rule, StaticRule):
        return rule
    return StaticRule(int(rule[0]), int(rule[1]))


GROUND_OBSTACLE, GROUND_GROUND, GROUND_IGNORED = 0, 1, 2   # ICPMI_GROUND_*
GROUND_MAX_BINS = 20400                                    # ICPMI_GROUND_MAX_BINS


class GroundConfig(C.Structure):
    """icpmi_ground_config"""
    _fields_ = [("n_rings", C.c_int32), ("n_sectors", C.c_int32), ("min_range", C.c_double), ("max_range", C.c_double),
                ("sensor_height", C.c_double), ("max_slope", C.c_double), ("step_tol", C.c_double),
                ("height_tol", C.c_double), ("clear_min", C.c_double), ("clear_max", C.c_double)]


class GroundInfo(C.Structure):
    """icpmi_ground_info"""
    _fields_ = [("n_ground", C.c_int64), ("n_obstacle", C.c_int64), ("n_ignored", C.c_int64),
                ("bins_accepted", C.c_int64)]


DESKEW_TIMES, DESKEW_AZIMUTH = 0, 1                       # ICPMI_DESKEW_*


class DeskewConfig(C.Structure):
    """icpmi_deskew_config"""
    _fields_ = [("twist", C.c_double * 6), ("t_ref", C.c_double), ("time_source", C.c_int32), ("direction", C.c_int32),
                ("azimuth_start", C.c_double), ("reserved", C.c_double * 4)]


class LocalMapConfig(C.Structure):
    """icpmi_local_map_config (defaults: local_map.LocalMapConfig)"""
    _fields_ = [("voxel_size", C.c_double), ("max_range", C.c_double), ("capacity", C.c_int64)]


class LocalMapInfo(C.Structure):
    """icpmi_local_map_info: the table's rows after an add, and what the add did with the scan's rows and the residents"""
    _fields_ = [("rows", C.c_int64), ("inserted", C.c_int64), ("evicted", C.c_int64), ("dropped", C.c_int64),
                ("merged", C.c_int64)]


class PoseGraphConfig(C.Structure):
    """slam::PoseGraphConfig (pose_graph.hpp:22-40)"""
    _fields_ = [("odom_rotation_sigma", C.c_double), ("odom_translation_sigma", C.c_double),
                ("prior_rotation_sigma", C.c_double), ("prior_translation_sigma", C.c_double),
                ("loop_rotation_sigma", C.c_double), ("loop_translation_sigma", C.c_double),
                ("max_iterations", C.c_int32), ("reserved", C.c_int32),
                ("relative_error_tol", C.c_double), ("absolute_error_tol", C.c_double)]


class PoseGraphInfo(C.Structure):
    _fields_ = [("optimized", C.c_int32), ("iterations", C.c_int32), ("inner_iterations", C.c_int32),
                ("stop_reason", C.c_int32), ("initial_error", C.c_double), ("final_error", C.c_double),
                ("final_lambda", C.c_double), ("history_len", C.c_int32), ("reserved", C.c_int32)]


PG_STOP_NONE, PG_STOP_ZERO_ERROR, PG_STOP_MAX_ITERATIONS, PG_STOP_RELATIVE, PG_STOP_ABSOLUTE, PG_STOP_LAMBDA_BOUND, \
    PG_STOP_SMALL_COST_CHANGE, PG_STOP_NOT_FINITE = range(8)
# a robust loss on the pose graph's loop-closure edges (ICPMI_PG_LOSS_*)
PG_LOSS_NONE, PG_LOSS_HUBER, PG_LOSS_CAUCHY, PG_LOSS_GEMAN_MCCLURE = range(4)


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int32)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int32)


class IcpError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("icp_mi355x error %d: %s" % (code, message))
        self.code = code


_LIB = None


def hip_runtimes_mapped(maps_text=None):
    """Distinct libamdhip64 images mapped into this process (real paths), from /proc/self/maps."""
    if maps_text is None:
        try:
            with open("/proc/self/maps") as f:
                maps_text = f.read()
        except OSError:
            return []
    seen = []
    for line in maps_text.splitlines():
        parts = line.split(None, 5)
        if len(parts) == 6 and os.path.basename(parts[5]).startswith("libamdhip64"):
            path = parts[5].strip()
            if path not in seen:
                seen.append(path)
    return seen


def _one_hip_runtime(before_dlopen):
    """One HIP runtime per process.  libicp_mi355x.so needs `libamdhip64.so.7`; the torch wheel
    bundles its own copy (SONAME libamdhip64.so.7, but torch's libraries ask for it as
    `libamdhip64.so`, which the dynamic loader does not recognise as the image /opt/rocm already
    provided).  Library first, torch second therefore maps TWO runtimes, and the first stream or
    event handed from one to the other aborts the process (`std::bad_variant_access`).  Torch
    first, library second resolves both to torch's copy.  So: import torch before the dlopen if
    it is there to be imported, and refuse to go on if two runtimes are mapped anyway."""
    import sys
    if before_dlopen:
        if "torch" not in sys.modules:
            import importlib.util
            if importlib.util.find_spec("torch") is not None:
                import torch  # noqa: F401
        return
    mapped = hip_runtimes_mapped()
    if len(mapped) > 1:
        raise IcpError(ERR_HIP, "two HIP runtimes are mapped into this process (%s): libicp_mi355x.so must "
                                "share torch's; import torch before anything loads /opt/rocm's libamdhip64"
                       % ", ".join(mapped))


def load_library(path=None):
    """dlopen the in-tree libicp_mi355x.so (must have been built: see build.build_library)."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    path = path or _build.LIB_PATH
    if not os.path.exists(path):
        raise FileNotFoundError(
            "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback)" % path)
    _one_hip_runtime(before_dlopen=True)
    L = C.CDLL(path)
    _one_hip_runtime(before_dlopen=False)
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    L.icpmi_version.restype = C.c_char_p
    L.icpmi_options_default.argtypes = [C.POINTER(Options)]
    L.icpmi_config_default.argtypes = [C.POINTER(Config)]
    L.icpmi_create.argtypes = [C.POINTER(Options), C.POINTER(vp)]
    L.icpmi_destroy.argtypes = [vp]
    L.icpmi_destroy.restype = None
    L.icpmi_last_error.argtypes = [vp]
    L.icpmi_last_error.restype = C.c_char_p
    L.icpmi_align.argtypes = [vp, dp, C.c_int64, dp, C.c_int64, C.POINTER(Config),
                              C.POINTER(Result), dp, C.c_int32]
    L.icpmi_align_device.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.POINTER(Config),
                                     C.POINTER(Result), dp, C.c_int32]
    L.icpmi_align_batch.argtypes = [vp, C.c_int32, C.POINTER(dp), C.POINTER(C.c_int64), C.POINTER(dp), C.POINTER(C.c_int64),
                                    C.POINTER(Config), C.POINTER(Result), dp, C.c_int32, C.POINTER(C.c_int32)]
    L.icpmi_align_gated.argtypes = [vp, dp, C.c_int64, dp, C.c_int64, C.POINTER(Config), C.POINTER(Gate),
                                    C.POINTER(Result), C.POINTER(GateInfo), dp, C.c_int32]
    L.icpmi_align_gated_device.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.POINTER(Config), C.POINTER(Gate),
                                           C.POINTER(Result), C.POINTER(GateInfo), dp, C.c_int32]
    L.icpmi_align_gated_batch.argtypes = [vp, C.c_int32, C.POINTER(dp), C.POINTER(C.c_int64), C.POINTER(dp), C.POINTER(C.c_int64),
                                          C.POINTER(Config), C.POINTER(Gate), C.POINTER(Result), C.POINTER(GateInfo), dp,
                                          C.c_int32, C.POINTER(C.c_int32)]
    L.icpmi_align_robust.argtypes = [vp, dp, C.c_int64, dp, C.c_int64, C.POINTER(Config), C.POINTER(Robust),
                                     C.POINTER(Result), C.POINTER(RobustInfo), dp, C.c_int32]
    L.icpmi_align_robust_device.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.POINTER(Config), C.POINTER(Robust),
                                            C.POINTER(Result), C.POINTER(RobustInfo), dp, C.c_int32]
    L.icpmi_align_robust_batch.argtypes = [vp, C.c_int32, C.POINTER(dp), C.POINTER(C.c_int64), C.POINTER(dp), C.POINTER(C.c_int64),
                                           C.POINTER(Config), C.POINTER(Robust), C.POINTER(Result), C.POINTER(RobustInfo), dp,
                                           C.c_int32, C.POINTER(C.c_int32)]
    L.icpmi_align_gicp.argtypes = [vp, dp, C.c_int64, dp, C.c_int64, C.POINTER(Config), C.POINTER(Gicp),
                                   C.POINTER(Result), C.POINTER(GicpInfo), dp, C.c_int32]
    L.icpmi_align_gicp_device.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.POINTER(Config), C.POINTER(Gicp),
                                          C.POINTER(Result), C.POINTER(GicpInfo), dp, C.c_int32]
    L.icpmi_align_gicp_batch.argtypes = [vp, C.c_int32, C.POINTER(dp), C.POINTER(C.c_int64), C.POINTER(dp), C.POINTER(C.c_int64),
                                         C.POINTER(Config), C.POINTER(Gicp), C.POINTER(Result), C.POINTER(GicpInfo), dp,
                                         C.c_int32, C.POINTER(C.c_int32)]
    L.icpmi_loop_set_gicp.argtypes = [vp, C.c_double]
    L.icpmi_stream_set_robust.argtypes = [vp, C.POINTER(Robust)]
    L.icpmi_stream_last_robust.argtypes = [vp, C.POINTER(RobustInfo)]
    L.icpmi_nearest_batch.argtypes = [vp, dp, C.c_int64, dp, C.c_int64, C.POINTER(C.c_int32), dp]
    L.icpmi_k_nearest.argtypes = [vp, dp, C.c_int64, dp, C.c_int64, C.c_int32, C.POINTER(C.c_int32), dp]
    L.icpmi_estimate_normals.argtypes = [vp, dp, C.c_int64, C.c_int32, dp]
    L.icpmi_solve_point_to_plane.argtypes = [vp, dp, dp, dp, C.c_int64, dp]
    L.icpmi_transform_points.argtypes = [vp, dp, dp, C.c_int64, dp]
    i64p = C.POINTER(C.c_int64)
    L.icpmi_voxel_downsample.argtypes = [vp, dp, C.c_int64, C.c_double, dp, C.c_int64, i64p]
    L.icpmi_voxel_downsample_device.argtypes = [vp, vp, C.c_int64, C.c_double, vp, C.c_int64, i64p]
    L.icpmi_load_cloud.argtypes = [C.c_char_p, dp, C.c_int64, i64p]
    L.icpmi_load_cloud_device.argtypes = [vp, C.c_char_p, vp, C.c_int64, i64p]
    L.icpmi_upload_points_f32.argtypes = [vp, C.POINTER(C.c_float), C.c_int64, C.c_int32, vp]
    L.icpmi_discover_frames.argtypes = [C.c_char_p, i64p, C.c_int64, C.c_char_p, C.c_int64, i64p, i64p]
    L.icpmi_estimate_normals_rows.argtypes = [vp, dp, C.c_int64, C.c_int32, C.c_int64, C.c_int64, dp]
    L.icpmi_stream_push.argtypes = [vp, vp, C.c_int64, C.c_double, C.c_int64, C.POINTER(Config), C.POINTER(Result), dp,
                                    C.c_int32, C.POINTER(StreamInfo)]
    L.icpmi_stream_push_host.argtypes = [vp, dp, C.c_int64, C.c_double, C.c_int64, C.POINTER(Config), C.POINTER(Result), dp,
                                         C.c_int32, C.POINTER(StreamInfo)]
    L.icpmi_stream_push_file.argtypes = [vp, C.c_char_p, C.c_double, C.c_int64, C.POINTER(Config), C.POINTER(Result), dp,
                                         C.c_int32, C.POINTER(StreamInfo)]
    L.icpmi_stream_reset.argtypes = [vp]
    L.icpmi_stream_prefetch_file.argtypes = [vp, C.c_char_p]
    L.icpmi_grid_config_default.argtypes = [C.POINTER(GridConfig)]
    L.icpmi_grid_config_default.restype = None
    L.icpmi_occupancy_update.argtypes = [vp, dp, C.c_int64, dp, C.POINTER(GridConfig), i64p]
    L.icpmi_occupancy_update_device.argtypes = [vp, vp, C.c_int64, dp, C.POINTER(GridConfig), i64p]
    L.icpmi_occupancy_cells.argtypes = [vp, C.POINTER(C.c_int32), C.c_int64, i64p]
    L.icpmi_occupancy_clear.argtypes = [vp]
    L.icpmi_stream_map_update.argtypes = [vp, dp, C.POINTER(GridConfig), dp, C.c_int64, i64p, i64p]
    L.icpmi_stream_current_scan.argtypes = [vp, dp, C.c_int64, i64p]
    L.icpmi_scan_context.argtypes = [vp, dp, C.c_int64, dp]
    L.icpmi_scan_context_distances.argtypes = [vp, dp, dp, C.c_int64, dp]
    L.icpmi_scan_context_distances_shift.argtypes = [vp, dp, dp, C.c_int64, dp, C.POINTER(C.c_int32)]
    L.icpmi_sc_shift_transform.argtypes = [C.c_int32, dp]
    L.icpmi_comm_unique_id.argtypes = [vp, vp]
    L.icpmi_comm_init.argtypes = [vp, C.c_int32, C.c_int32, vp]
    L.icpmi_comm_finalize.argtypes = [vp]
    L.icpmi_comm_init_callbacks.argtypes = [vp, C.c_int32, C.c_int32, ALLREDUCE_FN, ALLGATHER_FN, vp]
    L.icpmi_comm_info.argtypes = [vp, C.POINTER(CommInfo)]
    L.icpmi_reset_profile.argtypes = [vp]
    L.icpmi_get_profile.argtypes = [vp, C.POINTER(Profile)]
    pg = C.c_void_p
    L.icpmi_pose_graph_config_default.argtypes = [C.POINTER(PoseGraphConfig)]
    L.icpmi_pose_graph_config_default.restype = None
    L.icpmi_pose_graph_create.argtypes = [vp, C.POINTER(PoseGraphConfig), C.POINTER(pg)]
    L.icpmi_pose_graph_destroy.argtypes = [pg]
    L.icpmi_pose_graph_destroy.restype = None
    L.icpmi_pose_graph_add_prior.argtypes = [pg, C.c_int64, dp]
    L.icpmi_pose_graph_add_odometry.argtypes = [pg, C.c_int64, C.c_int64, dp, C.c_double]
    L.icpmi_pose_graph_add_loop_closure.argtypes = [pg, C.c_int64, C.c_int64, dp]
    L.icpmi_pose_graph_optimize.argtypes = [pg, C.POINTER(PoseGraphInfo), dp, C.c_int32]
    L.icpmi_pose_graph_pose.argtypes = [pg, C.c_int64, dp]
    L.icpmi_pose_graph_poses.argtypes = [pg, dp, C.c_int64, i64p, i64p]
    L.icpmi_pose_graph_size.argtypes = [pg, i64p, i64p, C.POINTER(PoseGraphInfo)]
    L.icpmi_pose_graph_set_loop_loss.argtypes = [pg, C.c_int32, C.c_double]
    L.icpmi_pose_graph_loop_loss.argtypes = [pg, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.icpmi_pose_graph_loop_weights.argtypes = [pg, dp, dp, C.c_int64, i64p]
    L.icpmi_pose_graph_add_odometry_information.argtypes = [pg, C.c_int64, C.c_int64, dp, dp]
    L.icpmi_pose_graph_add_loop_closure_information.argtypes = [pg, C.c_int64, C.c_int64, dp, dp]
    L.icpmi_pose_graph_marginals.argtypes = [pg, i64p, C.c_int32, dp]
    L.icpmi_pose_graph_relative_covariance.argtypes = [pg, C.c_int64, C.c_int64, dp]
    L.icpmi_pose_graph_closure_distance.argtypes = [pg, C.c_int64, C.c_int64, dp, dp, dp]
    L.icpmi_information_from_icp.argtypes = [dp, dp, C.c_double, C.c_double, C.c_double, dp]
    L.icpmi_last_normal_matrix.argtypes = [vp, C.c_int32, C.POINTER(NormalMatrix)]
    L.icpmi_map_create.argtypes = [vp, C.POINTER(vp)]
    L.icpmi_map_destroy.argtypes = [vp]
    L.icpmi_map_destroy.restype = None
    L.icpmi_map_add_frame.argtypes = [vp, dp, C.c_int64]
    L.icpmi_map_add_frame_device.argtypes = [vp, vp, C.c_int64]
    L.icpmi_map_add_stream_frame.argtypes = [vp]
    L.icpmi_map_size.argtypes = [vp, i64p, i64p]
    L.icpmi_map_world.argtypes = [vp, dp, C.c_int64, C.c_int64, dp, C.c_int64, i64p]
    L.icpmi_map_finish.argtypes = [vp, dp, C.c_int64, C.POINTER(GridConfig), C.c_double, dp, C.c_int64, i64p, i64p]
    L.icpmi_map_raycast.argtypes = [vp, dp, C.c_int64, C.POINTER(GridConfig), C.POINTER(RasterInfo)]
    L.icpmi_map_raster.argtypes = [vp, C.POINTER(C.c_int8), C.c_int64, C.POINTER(RasterInfo)]
    L.icpmi_map_raycast_counts.argtypes = [vp, dp, C.c_int64, C.POINTER(GridConfig), C.POINTER(CountsInfo)]
    L.icpmi_map_counts.argtypes = [vp, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.POINTER(C.c_int8), C.c_int64,
                                   C.POINTER(CountsInfo)]
    L.icpmi_map_live_update.argtypes = [vp, dp, C.c_int64, C.POINTER(GridConfig), C.POINTER(LiveInfo)]
    L.icpmi_map_live_counts.argtypes = [vp, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.POINTER(C.c_int8), C.c_int64,
                                        C.POINTER(LiveInfo)]
    L.icpmi_map_live_clear.argtypes = [vp]
    u8p = C.POINTER(C.c_uint8)
    L.icpmi_ground_config_default.argtypes = [C.POINTER(GroundConfig)]
    L.icpmi_ground_config_default.restype = None
    L.icpmi_ground_segment.argtypes = [vp, dp, C.c_int64, C.POINTER(GroundConfig), u8p, dp, dp, C.POINTER(GroundInfo)]
    L.icpmi_ground_segment_device.argtypes = [vp, vp, C.c_int64, C.POINTER(GroundConfig), u8p, dp, dp, C.POINTER(GroundInfo)]
    L.icpmi_map_set_ground.argtypes = [vp, C.POINTER(GroundConfig)]
    L.icpmi_map_ground_labels.argtypes = [vp, C.c_int64, u8p, C.c_int64, i64p]
    L.icpmi_map_world_static.argtypes = [vp, dp, C.c_int64, C.POINTER(GridConfig), C.POINTER(StaticRule), C.c_int64, dp, C.c_int64,
                                         i64p, C.POINTER(StaticInfo)]
    L.icpmi_map_finish_static.argtypes = [vp, dp, C.c_int64, C.POINTER(GridConfig), C.POINTER(StaticRule), C.c_double, dp, C.c_int64,
                                          i64p, C.POINTER(StaticInfo)]
    L.icpmi_map_static_labels.argtypes = [vp, C.c_int64, u8p, C.c_int64, i64p]
    L.icpmi_deskew_config_default.argtypes = [C.POINTER(DeskewConfig)]
    L.icpmi_deskew_config_default.restype = None
    L.icpmi_deskew.argtypes = [vp, dp, dp, C.c_int64, C.POINTER(DeskewConfig), dp]
    L.icpmi_deskew_device.argtypes = [vp, vp, vp, C.c_int64, C.POINTER(DeskewConfig), vp]
    L.icpmi_deskew_twist.argtypes = [dp, dp]
    L.icpmi_stream_set_deskew.argtypes = [vp, C.POINTER(DeskewConfig)]
    L.icpmi_loop_config_default.argtypes = [C.POINTER(LoopConfig)]
    L.icpmi_loop_config_default.restype = None
    L.icpmi_loop_create.argtypes = [vp, C.POINTER(LoopConfig), C.POINTER(vp)]
    L.icpmi_loop_destroy.argtypes = [vp]
    L.icpmi_loop_destroy.restype = None
    L.icpmi_loop_add_frame.argtypes = [vp, C.c_int64, C.c_int32]
    L.icpmi_loop_detect.argtypes = [vp, C.POINTER(LoopResult), C.c_int64, i64p]
    L.icpmi_loop_descriptor.argtypes = [vp, C.c_int64, dp]
    L.icpmi_loop_size.argtypes = [vp, i64p]
    L.icpmi_loop_clear.argtypes = [vp]
    L.icpmi_loop_set_yaw_guess.argtypes = [vp, C.c_int32]
    L.icpmi_loop_last_shifts.argtypes = [vp, C.POINTER(C.c_int32), C.c_int64, i64p]
    L.icpmi_loop_set_gate.argtypes = [vp, C.c_double]
    L.icpmi_loop_last_pairs.argtypes = [vp, i64p, C.c_int64, i64p]
    L.icpmi_loop_set_robust.argtypes = [vp, C.c_int32, C.c_double]
    L.icpmi_loop_last_weights.argtypes = [vp, dp, C.c_int64, i64p]
    L.icpmi_loop_set_information.argtypes = [vp, C.c_double, C.c_double, C.c_double]
    L.icpmi_loop_last_information.argtypes = [vp, dp, C.c_int64, i64p]
    L.icpmi_local_map_config_default.argtypes = [C.POINTER(LocalMapConfig)]
    L.icpmi_local_map_config_default.restype = None
    L.icpmi_local_map_create.argtypes = [vp, C.POINTER(LocalMapConfig), C.POINTER(vp)]
    L.icpmi_local_map_destroy.argtypes = [vp]
    L.icpmi_local_map_destroy.restype = None
    L.icpmi_local_map_clear.argtypes = [vp]
    L.icpmi_local_map_add.argtypes = [vp, dp, C.c_int64, dp, C.POINTER(LocalMapInfo)]
    L.icpmi_local_map_add_device.argtypes = [vp, vp, C.c_int64, dp, C.POINTER(LocalMapInfo)]
    L.icpmi_local_map_add_stream_frame.argtypes = [vp, dp, C.POINTER(LocalMapInfo)]
    L.icpmi_local_map_size.argtypes = [vp, i64p]
    L.icpmi_local_map_points.argtypes = [vp, dp, C.POINTER(C.c_uint64), C.c_int64, i64p]
    L.icpmi_local_map_register.argtypes = [vp, dp, C.c_int64, C.POINTER(Config), C.POINTER(Result), dp, C.c_int32]
    L.icpmi_local_map_register_device.argtypes = [vp, vp, C.c_int64, C.POINTER(Config), C.POINTER(Result), dp, C.c_int32]
    L.icpmi_local_map_register_robust.argtypes = [vp, dp, C.c_int64, C.POINTER(Config), C.POINTER(Robust), C.POINTER(Result),
                                                  C.POINTER(RobustInfo), dp, C.c_int32]
    L.icpmi_local_map_register_robust_device.argtypes = [vp, vp, C.c_int64, C.POINTER(Config), C.POINTER(Robust),
                                                         C.POINTER(Result), C.POINTER(RobustInfo), dp, C.c_int32]
    for name in EXPORTS:
        getattr(L, name)  # raises AttributeError if a declared symbol is not exported
    _LIB = L
    return L


def load_cloud(path):
    """load_ply / load_bin (file_utils.cpp:20-141) through the library: N x 3 fp64."""
    L = load_library()
    n = C.c_int64(0)
    rc = L.icpmi_load_cloud(os.fsencode(path), None, 0, C.byref(n))
    if rc != OK:
        raise IcpError(rc, L.icpmi_last_error(None).decode())
    out = np.empty((n.value, 3))
    rc = L.icpmi_load_cloud(os.fsencode(path), out.ctypes.data_as(C.POINTER(C.c_double)), n.value, C.byref(n))
    if rc != OK:
        raise IcpError(rc, L.icpmi_last_error(None).decode())
    return out


def discover_frames(data_dir):
    """discover_frames (file_utils.cpp:217-247) through the library -> [(number, path), ...] sorted by number."""
    L = load_library()
    n, nbytes = C.c_int64(0), C.c_int64(0)
    rc = L.icpmi_discover_frames(os.fsencode(data_dir), None, 0, None, 0, C.byref(n), C.byref(nbytes))
    if rc != OK:
        raise IcpError(rc, L.icpmi_last_error(None).decode())
    if n.value == 0:
        return []
    stamps = (C.c_int64 * n.value)()
    buf = C.create_string_buffer(nbytes.value)
    rc = L.icpmi_discover_frames(os.fsencode(data_dir), stamps, n.value, buf, nbytes.value, C.byref(n), C.byref(nbytes))
    if rc != OK:
        raise IcpError(rc, L.icpmi_last_error(None).decode())
    paths = buf.raw[:nbytes.value].split(b"\0")[:n.value]
    return [(int(stamps[i]), os.fsdecode(paths[i])) for i in range(n.value)]


def _f64(a, cols=3):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if cols and (a.ndim != 2 or a.shape[1] != cols):
        raise ValueError("expected an N x %d array" % cols)
    return a


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def information_from_icp(JtJ, T, sigma, floor_rotation_sigma=0.0, floor_translation_sigma=0.0):
    """icpmi_information_from_icp: the 6 x 6 information of a pose-graph edge entered as rel = T (from the target's pose
    to the source's) from the normal matrix JtJ of the registration that gave T.  sigma: the residual noise of one pair
    in metres; the floors (0: none) are sigmas of an isotropic term that keeps a rank-deficient JtJ positive definite.
    A pure host function: no context, no device."""
    J = np.ascontiguousarray(JtJ, dtype=np.float64)
    Tm = np.ascontiguousarray(T, dtype=np.float64)
    if J.shape != (6, 6) or Tm.shape != (4, 4):
        raise ValueError("expected a 6 x 6 normal matrix and a 4 x 4 transform")
    out = np.zeros((6, 6))
    rc = load_library().icpmi_information_from_icp(_dp(J), _dp(Tm), float(sigma), float(floor_rotation_sigma),
                                                   float(floor_translation_sigma), _dp(out))
    if rc != OK:
        raise IcpError(rc, "information_from_icp: sigma must be finite and > 0, a floor 0 or finite and > 0, and "
                           "JtJ and T finite")
    return out


class Context:
    """One icpmi_ctx: a device, a stream and its workspace."""

    def __init__(self, device=0, normal_k=20, search=SEARCH_AUTO, profile=False):
        self._lib = load_library()
        opt = Options()
        self._lib.icpmi_options_default(C.byref(opt))
        opt.device, opt.normal_k, opt.search, opt.profile = device, normal_k, search, int(profile)
        h = C.c_void_p()
        rc = self._lib.icpmi_create(C.byref(opt), C.byref(h))
        if rc != OK:
            raise IcpError(rc, self._lib.icpmi_last_error(None).decode())
        self._h = h
        self.n_ranks, self.rank = 1, 0

    def close(self):
        if getattr(self, "_h", None):
            for g in list(getattr(self, "_pose_graphs", ())):   # icpmi_pose_graph handles go before their context
                g.close()
            for d in list(getattr(self, "_loops", ())):         # icpmi_loop handles go before their maps
                d.close()
            for m in list(getattr(self, "_maps", ())):          # ... and so do icpmi_map handles
                m.close()
            for m in list(getattr(self, "_local_maps", ())):    # ... and icpmi_local_map handles
                m.close()
            self._lib.icpmi_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        if rc != OK:
            raise IcpError(rc, self._lib.icpmi_last_error(self._h).decode())

    @staticmethod
    def make_config(max_iterations=50, tolerance=1e-6, min_error=1e-9, initial_transform=None):
        cfg = Config()
        cfg.max_iterations, cfg.tolerance, cfg.min_error = int(max_iterations), tolerance, min_error
        it = np.eye(4) if initial_transform is None else np.asarray(initial_transform, dtype=np.float64)
        for i, v in enumerate(it.reshape(16)):
            cfg.initial_transform[i] = v
        return cfg

    def align(self, source, target, cfg):
        src, tgt = _f64(source), _f64(target)
        cap = cfg.max_iterations + 1
        hist = np.zeros(max(cap, 1))
        res = Result()
        self._check(self._lib.icpmi_align(self._h, _dp(src), src.shape[0], _dp(tgt), tgt.shape[0],
                                          C.byref(cfg), C.byref(res), _dp(hist), cap))
        return res, hist[:res.history_len].copy()

    def align_batch(self, sources, targets, cfgs):
        """Several independent registrations at once (icpmi_align_batch: the verifications of one
        LoopClosureDetector::detect, loop_closure.hpp:94-123) -> [(Result, error history), ...], each
        bit-identical to align() of the same pair.  cfgs: one Config for all, or one per pair."""
        srcs, tgts = [_f64(a) for a in sources], [_f64(a) for a in targets]
        k = len(srcs)
        if k != len(tgts) or k < 1:
            raise ValueError("as many targets as sources, at least one")
        cfg_list = list(cfgs) if isinstance(cfgs, (list, tuple)) else [cfgs] * k
        cfg_arr = (Config * k)(*cfg_list)
        stride = max(c.max_iterations for c in cfg_list) + 1
        hist = np.zeros((k, stride))
        res = (Result * k)()
        status = (C.c_int32 * k)()
        dpp = C.POINTER(C.c_double)
        sp = (dpp * k)(*[_dp(a) for a in srcs])
        tp = (dpp * k)(*[_dp(a) for a in tgts])
        ns = (C.c_int64 * k)(*[a.shape[0] for a in srcs])
        nt = (C.c_int64 * k)(*[a.shape[0] for a in tgts])
        self._check(self._lib.icpmi_align_batch(self._h, k, sp, ns, tp, nt, cfg_arr, res, _dp(hist), stride, status))
        out = []
        for i in range(k):
            r = Result()
            C.memmove(C.byref(r), C.byref(res[i]), C.sizeof(Result))
            out.append((r, hist[i, :r.history_len].copy()))
        return out

    def last_normal_matrix(self, k=0):
        """icpmi_last_normal_matrix: the normal equations of the pass that produced final_error of the last registration
        this context ran (problem k of the last batch call) -> an object with JtJ (6 x 6), Jtb (6), sum_sq, weight, pairs
        and T (4 x 4).  Raises IcpError(ERR_ARG) where no registration ran or its last pass kept no row."""
        nm = NormalMatrix()
        self._check(self._lib.icpmi_last_normal_matrix(self._h, int(k), C.byref(nm)))

        class _N:
            pass

        out = _N()
        out.JtJ = np.array(nm.JtJ[:]).reshape(6, 6)
        out.Jtb = np.array(nm.Jtb[:])
        out.sum_sq, out.weight, out.pairs = float(nm.sum_sq), float(nm.weight), int(nm.pairs)
        out.T = np.array(nm.T[:]).reshape(4, 4)
        return out

    def align_device(self, src_ptr, n_src, tgt_ptr, n_tgt, cfg):
        """src_ptr/tgt_ptr: device addresses of row-major N x 3 fp64 (e.g. tensor.data_ptr())."""
        cap = cfg.max_iterations + 1
        hist = np.zeros(max(cap, 1))
        res = Result()
        self._check(self._lib.icpmi_align_device(self._h, C.c_void_p(src_ptr), n_src,
                                                 C.c_void_p(tgt_ptr), n_tgt, C.byref(cfg),
                                                 C.byref(res), _dp(hist), cap))
        return res, hist[:res.history_len].copy()

    @staticmethod
    def _gate(max_distance):
        g = Gate()
        g.max_distance = float(max_distance)
        return g

    def align_gated(self, source, target, cfg, max_distance):
        """align() behind a correspondence-distance gate (icpmi_align_gated): a pass sums only the rows whose nearest
        target is within max_distance -> (Result, error history, rows kept by the pass that produced final_error)"""
        src, tgt = _f64(source), _f64(target)
        cap = cfg.max_iterations + 1
        hist = np.zeros(max(cap, 1))
        res, info, gate = Result(), GateInfo(), self._gate(max_distance)
        self._check(self._lib.icpmi_align_gated(self._h, _dp(src), src.shape[0], _dp(tgt), tgt.shape[0], C.byref(cfg),
                                                C.byref(gate), C.byref(res), C.byref(info), _dp(hist), cap))
        return res, hist[:res.history_len].copy(), int(info.pairs)

    def align_gated_device(self, src_ptr, n_src, tgt_ptr, n_tgt, cfg, max_distance):
        """align_gated with both clouds in device memory (addresses of row-major N x 3 fp64)"""
        cap = cfg.max_iterations + 1
        hist = np.zeros(max(cap, 1))
        res, info, gate = Result(), GateInfo(), self._gate(max_distance)
        self._check(self._lib.icpmi_align_gated_device(self._h, C.c_void_p(src_ptr), n_src, C.c_void_p(tgt_ptr), n_tgt,
                                                       C.byref(cfg), C.byref(gate), C.byref(res), C.byref(info),
                                                       _dp(hist), cap))
        return res, hist[:res.history_len].copy(), int(info.pairs)

    def align_gated_batch(self, sources, targets, cfgs, max_distances):
        """align_batch behind a gate (icpmi_align_gated_batch) -> [(Result, error history, pairs), ...], each
        bit-identical to align_gated() of the same pair.  max_distances: one for all, or one per pair."""
        srcs, tgts = [_f64(a) for a in sources], [_f64(a) for a in targets]
        k = len(srcs)
        if k != len(tgts) or k < 1:
            raise ValueError("as many targets as sources, at least one")
        cfg_list = list(cfgs) if isinstance(cfgs, (list, tuple)) else [cfgs] * k
        gate_list = list(max_distances) if isinstance(max_distances, (list, tuple)) else [max_distances] * k
        cfg_arr = (Config * k)(*cfg_list)
        gates = (Gate * k)(*[self._gate(g) for g in gate_list])
        stride = max(c.max_iterations for c in cfg_list) + 1
        hist = np.zeros((k, stride))
        res, infos = (Result * k)(), (GateInfo * k)()
        status = (C.c_int32 * k)()
        dpp = C.POINTER(C.c_double)
        sp = (dpp * k)(*[_dp(a) for a in srcs])
        tp = (dpp * k)(*[_dp(a) for a in tgts])
        ns = (C.c_int64 * k)(*[a.shape[0] for a in srcs])
        nt = (C.c_int64 * k)(*[a.shape[0] for a in tgts])
        self._check(self._lib.icpmi_align_gated_batch(self._h, k, sp, ns, tp, nt, cfg_arr, gates, res, infos, _dp(hist),
                                                      stride, status))
        out = []
        for i in range(k):
            r = Result()
            C.memmove(C.byref(r), C.byref(res[i]), C.sizeof(Result))
            out.append((r, hist[i, :r.history_len].copy(), int(infos[i].pairs)))
        return out

    def align_robust(self, source, target, cfg, rule):
        """align() under robust row weights (icpmi_align_robust; rule: see as_robust) -> (Result, error history,
        RobustInfo).  final_error and the history are the WEIGHTED RMS, which reads lower than the plain one."""
        src, tgt = _f64(source), _f64(target)
        cap = cfg.max_iterations + 1
        hist = np.zeros(max(cap, 1))
        res, info, r = Result(), RobustInfo(), as_robust(rule)
        self._check(self._lib.icpmi_align_robust(self._h, _dp(src), src.shape[0], _dp(tgt), tgt.shape[0], C.byref(cfg),
                                                 C.byref(r), C.byref(res), C.byref(info), _dp(hist), cap))
        return res, hist[:res.history_len].copy(), info

    def align_robust_device(self, src_ptr, n_src, tgt_ptr, n_tgt, cfg, rule):
        """align_robust with both clouds in device memory (addresses of row-major N x 3 fp64)"""
        cap = cfg.max_iterations + 1
        hist = np.zeros(max(cap, 1))
        res, info, r = Result(), RobustInfo(), as_robust(rule)
        self._check(self._lib.icpmi_align_robust_device(self._h, C.c_void_p(src_ptr), n_src, C.c_void_p(tgt_ptr), n_tgt,
                                                        C.byref(cfg), C.byref(r), C.byref(res), C.byref(info),
                                                        _dp(hist), cap))
        return res, hist[:res.history_len].copy(), info

    def align_gicp(self, source, target, cfg, rule):
        """align() with the plane-to-plane cost (icpmi_align_gicp; rule: see as_gicp) -> (Result, error history,
        GicpInfo).  final_error and the history read in metres (the header has the scaling)."""
        src, tgt = _f64(source), _f64(target)
        cap = cfg.max_iterations + 1
        hist = np.zeros(max(cap, 1))
        res, info, g = Result(), GicpInfo(), as_gicp(rule)
        self._check(self._lib.icpmi_align_gicp(self._h, _dp(src), src.shape[0], _dp(tgt), tgt.shape[0], C.byref(cfg),
                                               C.byref(g), C.byref(res), C.byref(info), _dp(hist), cap))
        return res, hist[:res.history_len].copy(), info

    def align_gicp_device(self, src_ptr, n_src, tgt_ptr, n_tgt, cfg, rule):
        """align_gicp with both clouds in device memory (addresses of row-major N x 3 fp64)"""
        cap = cfg.max_iterations + 1
        hist = np.zeros(max(cap, 1))
        res, info, g = Result(), GicpInfo(), as_gicp(rule)
        self._check(self._lib.icpmi_align_gicp_device(self._h, C.c_void_p(src_ptr), n_src, C.c_void_p(tgt_ptr), n_tgt,
                                                      C.byref(cfg), C.byref(g), C.byref(res), C.byref(info),
                                                      _dp(hist), cap))
        return res, hist[:res.history_len].copy(), info

    def align_robust_batch(self, sources, targets, cfgs, rules):
        """align_batch under row weights (icpmi_align_robust_batch) -> [(Result, error history, RobustInfo), ...], each
        bit-identical to align_robust() of the same pair.  rules: one for all (a Robust or a tuple), or a list, one per
        pair."""
        return self._align_rule_batch(self._lib.icpmi_align_robust_batch, Robust, RobustInfo, as_robust, sources, targets, cfgs, rules)

    def align_gicp_batch(self, sources, targets, cfgs, rules):
        """align_batch with the plane-to-plane cost (icpmi_align_gicp_batch) -> [(Result, error history, GicpInfo), ...],
        each bit-identical to align_gicp() of the same pair.  rules: one for all (a Gicp or a tuple, see as_gicp), or a
        list, one per pair, each with its own form."""
        return self._align_rule_batch(self._lib.icpmi_align_gicp_batch, Gicp, GicpInfo, as_gicp, sources, targets, cfgs, rules)

    def _align_rule_batch(self, entry, Rule, Info, as_rule, sources, targets, cfgs, rules):
        srcs, tgts = [_f64(a) for a in sources], [_f64(a) for a in targets]
        k = len(srcs)
        if k != len(tgts) or k < 1:
            raise ValueError("as many targets as sources, at least one")
        cfg_list = list(cfgs) if isinstance(cfgs, (list, tuple)) else [cfgs] * k
        rule_list = list(rules) if isinstance(rules, list) else [rules] * k
        cfg_arr = (Config * k)(*cfg_list)
        rule_arr = (Rule * k)()
        for i, rule in enumerate(rule_list):
            C.memmove(C.byref(rule_arr[i]), C.byref(as_rule(rule)), C.sizeof(Rule))
        stride = max(c.max_iterations for c in cfg_list) + 1
        hist = np.zeros((k, stride))
        res, infos = (Result * k)(), (Info * k)()
        status = (C.c_int32 * k)()
        dpp = C.POINTER(C.c_double)
        sp = (dpp * k)(*[_dp(a) for a in srcs])
        tp = (dpp * k)(*[_dp(a) for a in tgts])
        ns = (C.c_int64 * k)(*[a.shape[0] for a in srcs])
        nt = (C.c_int64 * k)(*[a.shape[0] for a in tgts])
        self._check(entry(self._h, k, sp, ns, tp, nt, cfg_arr, rule_arr, res, infos, _dp(hist), stride, status))
        out = []
        for i in range(k):
            r, inf = Result(), Info()
            C.memmove(C.byref(r), C.byref(res[i]), C.sizeof(Result))
            C.memmove(C.byref(inf), C.byref(infos[i]), C.sizeof(Info))
            out.append((r, hist[i, :r.history_len].copy(), inf))
        return out

    def nearest_batch(self, targets, queries, want_dist=True):
        tgt, qry = _f64(targets), _f64(queries)
        idx = np.empty(qry.shape[0], dtype=np.int32)
        d2 = np.empty(qry.shape[0]) if want_dist else None
        self._check(self._lib.icpmi_nearest_batch(
            self._h, _dp(tgt), tgt.shape[0], _dp(qry), qry.shape[0],
            idx.ctypes.data_as(C.POINTER(C.c_int32)), _dp(d2) if want_dist else None))
        return idx, d2

    def k_nearest(self, targets, queries, k, want_dist=True):
        """kdtree.hpp:65-78 for a batch of queries -> (indices n x k closest first, squared distances)"""
        tgt, qry = _f64(targets), _f64(queries)
        idx = np.empty((qry.shape[0], k), dtype=np.int32)
        d2 = np.empty((qry.shape[0], k)) if want_dist else None
        self._check(self._lib.icpmi_k_nearest(
            self._h, _dp(tgt), tgt.shape[0], _dp(qry), qry.shape[0], k,
            idx.ctypes.data_as(C.POINTER(C.c_int32)), _dp(d2) if want_dist else None))
        return idx, d2

    def estimate_normals(self, points, k=20):
        pts = _f64(points)
        out = np.empty_like(pts)
        self._check(self._lib.icpmi_estimate_normals(self._h, _dp(pts), pts.shape[0], k, _dp(out)))
        return out

    def solve_point_to_plane(self, source, target, normals):
        s, t, n = _f64(source), _f64(target), _f64(normals)
        if not (s.shape == t.shape == n.shape):
            raise ValueError("source, target and normals must have the same shape")
        T = np.empty(16)
        self._check(self._lib.icpmi_solve_point_to_plane(self._h, _dp(s), _dp(t), _dp(n), s.shape[0], _dp(T)))
        return T.reshape(4, 4)

    def transform_points(self, T, points):
        pts = _f64(points)
        Tm = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
        out = np.empty_like(pts)
        self._check(self._lib.icpmi_transform_points(self._h, _dp(Tm), _dp(pts), pts.shape[0], _dp(out)))
        return out

    def voxel_downsample(self, points, voxel_size):
        """file_utils.cpp:148-196 on the GPU; voxels sorted by key."""
        pts = _f64(points)
        out = np.empty_like(pts)
        n_out = C.c_int64(0)
        self._check(self._lib.icpmi_voxel_downsample(self._h, _dp(pts), pts.shape[0], float(voxel_size),
                                                     _dp(out), pts.shape[0], C.byref(n_out)))
        return out[:n_out.value].copy()

    def voxel_downsample_device(self, src_ptr, n, voxel_size, out_ptr, out_cap):
        n_out = C.c_int64(0)
        self._check(self._lib.icpmi_voxel_downsample_device(self._h, C.c_void_p(src_ptr), n, float(voxel_size),
                                                            C.c_void_p(out_ptr), out_cap, C.byref(n_out)))
        return n_out.value

    def estimate_normals_rows(self, points, k, row0, row1):
        """icp.hpp:23-67 for rows [row0, row1) only (against the whole cloud)"""
        pts = _f64(points)
        out = np.empty((row1 - row0, 3))
        self._check(self._lib.icpmi_estimate_normals_rows(self._h, _dp(pts), pts.shape[0], k, row0, row1, _dp(out)))
        return out

    def upload_points_f32(self, records, out_ptr):
        """records: n x stride float32 (x, y, z leading) -> n x 3 fp64 at device address out_ptr"""
        rec = np.ascontiguousarray(records, dtype=np.float32)
        self._check(self._lib.icpmi_upload_points_f32(self._h, rec.ctypes.data_as(C.POINTER(C.c_float)), rec.shape[0],
                                                      rec.shape[1], C.c_void_p(out_ptr)))

    def load_cloud_device_rows(self, path):
        n = C.c_int64(0)
        self._check(self._lib.icpmi_load_cloud_device(self._h, os.fsencode(path), None, 0, C.byref(n)))
        return n.value

    def load_cloud_device(self, path, out_ptr, cap):
        """load_ply / load_bin (file_utils.cpp:20-141) straight into device memory; returns the row count"""
        n = C.c_int64(0)
        self._check(self._lib.icpmi_load_cloud_device(self._h, os.fsencode(path), C.c_void_p(out_ptr), cap, C.byref(n)))
        return n.value

    def stream_push(self, raw_ptr, n_raw, voxel, min_points, cfg):
        """slam_node.cpp:122-152 on resident clouds -> (Result, error history, StreamInfo)"""
        cap = cfg.max_iterations + 1
        hist = np.zeros(max(cap, 1))
        res, info = Result(), StreamInfo()
        self._check(self._lib.icpmi_stream_push(self._h, C.c_void_p(raw_ptr), n_raw, float(voxel), int(min_points),
                                                C.byref(cfg), C.byref(res), _dp(hist), cap, C.byref(info)))
        return res, hist[:res.history_len].copy(), info

    def stream_push_host(self, raw, voxel, min_points, cfg):
        """stream_push with the raw scan in host memory (N x 3 fp64)"""
        pts = _f64(raw)
        cap = cfg.max_iterations + 1
        hist = np.zeros(max(cap, 1))
        res, info = Result(), StreamInfo()
        self._check(self._lib.icpmi_stream_push_host(self._h, _dp(pts), pts.shape[0], float(voxel), int(min_points),
                                                     C.byref(cfg), C.byref(res), _dp(hist), cap, C.byref(info)))
        return res, hist[:res.history_len].copy(), info

    def stream_push_file(self, path, voxel, min_points, cfg):
        """stream_push with the raw scan in a file (.bin: disk -> pinned memory -> device as float32)"""
        cap = cfg.max_iterations + 1
        hist = np.zeros(max(cap, 1))
        res, info = Result(), StreamInfo()
        self._check(self._lib.icpmi_stream_push_file(self._h, os.fsencode(path), float(voxel), int(min_points),
                                                     C.byref(cfg), C.byref(res), _dp(hist), cap, C.byref(info)))
        return res, hist[:res.history_len].copy(), info

    def stream_prefetch_file(self, path):
        """start reading the NEXT frame file on the context's worker thread (call before pushing the current one)"""
        self._check(self._lib.icpmi_stream_prefetch_file(self._h, os.fsencode(path)))

    def stream_reset(self):
        self._check(self._lib.icpmi_stream_reset(self._h))

    def stream_set_robust(self, rule):
        """icpmi_stream_set_robust: every later stream_push* registers under the rule (see as_robust; None: off)"""
        if rule is None:
            self._check(self._lib.icpmi_stream_set_robust(self._h, None))
        else:
            self._check(self._lib.icpmi_stream_set_robust(self._h, C.byref(as_robust(rule))))

    def deskew(self, xyz, times, cfg):
        """icpmi_deskew: the n rows of xyz (N x 3 fp64, host) moved into the sensor frame at cfg.t_ref under cfg (a
        DeskewConfig structure); times: N doubles or None (ICPMI_DESKEW_AZIMUTH) -> N x 3"""
        pts = _f64(xyz) if len(xyz) else np.zeros((0, 3))
        t = None if times is None else np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        if t is not None and t.shape[0] != pts.shape[0]:
            raise ValueError("one time per row")
        out = np.empty_like(pts)
        self._check(self._lib.icpmi_deskew(self._h, _dp(pts), None if t is None else _dp(t), pts.shape[0], C.byref(cfg), _dp(out)))
        return out

    def deskew_device(self, xyz_ptr, times_ptr, n, cfg, out_ptr):
        """icpmi_deskew_device: the same on device memory, queued on the context's stream without a wait; out_ptr may be
        xyz_ptr; times_ptr None or 0 without times"""
        self._check(self._lib.icpmi_deskew_device(self._h, C.c_void_p(xyz_ptr), C.c_void_p(times_ptr or None), int(n),
                                                  C.byref(cfg), C.c_void_p(out_ptr)))

    def stream_set_deskew(self, cfg):
        """icpmi_stream_set_deskew: every later stream_push / stream_push_host deskews the raw scan under cfg (a
        DeskewConfig structure with time_source DESKEW_AZIMUTH; None: off) before it filters it"""
        self._check(self._lib.icpmi_stream_set_deskew(self._h, None if cfg is None else C.byref(cfg)))

    def stream_last_robust(self):
        """icpmi_stream_last_robust -> RobustInfo of the last push's registration (zeros without one, or without a rule)"""
        info = RobustInfo()
        self._check(self._lib.icpmi_stream_last_robust(self._h, C.byref(info)))
        return info

    @staticmethod
    def make_grid_config(resolution=None, height_min=None, height_max=None, max_range=None):
        g = GridConfig()
        load_library().icpmi_grid_config_default(C.byref(g))
        for name, v in (("resolution", resolution), ("height_min", height_min), ("height_max", height_max),
                        ("max_range", max_range)):
            if v is not None:
                setattr(g, name, float(v))
        return g

    def occupancy_update(self, world, sensor, grid=None):
        """update_occupancy_grid(world, sensor) (slam_node.cpp:211-221) into the context's cell set -> its size"""
        pts = _f64(world) if len(world) else np.zeros((0, 3))
        sx = np.ascontiguousarray(sensor, dtype=np.float64).reshape(3)
        g = grid if grid is not None else self.make_grid_config()
        n = C.c_int64(0)
        self._check(self._lib.icpmi_occupancy_update(self._h, _dp(pts), pts.shape[0], _dp(sx), C.byref(g), C.byref(n)))
        return n.value

    def occupancy_update_device(self, ptr, n_rows, sensor, grid=None):
        sx = np.ascontiguousarray(sensor, dtype=np.float64).reshape(3)
        g = grid if grid is not None else self.make_grid_config()
        n = C.c_int64(0)
        self._check(self._lib.icpmi_occupancy_update_device(self._h, C.c_void_p(ptr), n_rows, _dp(sx), C.byref(g), C.byref(n)))
        return n.value

    def occupancy_cells(self):
        """the set as an (n, 2) int32 array of (x, y), sorted by x then y"""
        n = C.c_int64(0)
        self._check(self._lib.icpmi_occupancy_cells(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 2), dtype=np.int32)
        if n.value:
            self._check(self._lib.icpmi_occupancy_cells(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), n.value, C.byref(n)))
        return out

    def occupancy_clear(self):
        self._check(self._lib.icpmi_occupancy_clear(self._h))

    def stream_current_scan(self):
        """the filtered scan the last stream_push* left resident (slam_node.cpp:122's `curr`), N x 3 fp64"""
        n = C.c_int64(0)
        self._check(self._lib.icpmi_stream_current_scan(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, 3))
        if n.value:
            self._check(self._lib.icpmi_stream_current_scan(self._h, _dp(out), n.value, C.byref(n)))
        return out

    def stream_map_update(self, pose, grid=None, want_world=True, update_grid=True, n_rows=None):
        """slam_node.cpp:147-153 on the scan the last stream_push* left resident: (world points or None, cells in the set).
        n_rows: the filtered scan's row count (info.n_filtered of the push), which saves asking the library for it."""
        T = np.ascontiguousarray(pose, dtype=np.float64).reshape(16)
        nw, nc = C.c_int64(0), C.c_int64(0)
        g = (grid if grid is not None else self.make_grid_config()) if update_grid else None
        world = None
        if want_world:
            if n_rows is None:
                self._check(self._lib.icpmi_stream_map_update(self._h, _dp(T), None, None, 0, C.byref(nw), C.byref(nc)))
                n_rows = nw.value
            world = np.empty((int(n_rows), 3))
        self._check(self._lib.icpmi_stream_map_update(self._h, _dp(T), C.byref(g) if g is not None else None,
                                                      _dp(world) if world is not None else None,
                                                      world.shape[0] if world is not None else 0, C.byref(nw), C.byref(nc)))
        return world, nc.value

    def scan_context(self, cloud):
        """scan_context.hpp:44-82 -> 20 x 60 descriptor"""
        pts = _f64(cloud)
        out = np.empty(1200)
        self._check(self._lib.icpmi_scan_context(self._h, _dp(pts), pts.shape[0], _dp(out)))
        return out.reshape(20, 60)

    def scan_context_distances(self, query_desc, hist_descs):
        """scan_context.hpp:90-142 for one query against a stack of descriptors"""
        q = np.ascontiguousarray(query_desc, dtype=np.float64).reshape(1200)
        h = np.ascontiguousarray(hist_descs, dtype=np.float64).reshape(-1, 1200)
        out = np.empty(h.shape[0])
        self._check(self._lib.icpmi_scan_context_distances(self._h, _dp(q), _dp(h), h.shape[0], _dp(out)))
        return out

    def scan_context_distances_shift(self, query_desc, hist_descs):
        """scan_context_distances and, per descriptor, the smallest column shift that attains its distance (int32)"""
        q = np.ascontiguousarray(query_desc, dtype=np.float64).reshape(1200)
        h = np.ascontiguousarray(hist_descs, dtype=np.float64).reshape(-1, 1200)
        out, shift = np.empty(h.shape[0]), np.empty(h.shape[0], dtype=np.int32)
        self._check(self._lib.icpmi_scan_context_distances_shift(self._h, _dp(q), _dp(h), h.shape[0], _dp(out),
                                                                 shift.ctypes.data_as(C.POINTER(C.c_int32))))
        return out, shift

    # multi-GPU
    def comm_unique_id(self):
        buf = C.create_string_buffer(UNIQUE_ID_BYTES)
        self._check(self._lib.icpmi_comm_unique_id(self._h, buf))
        return buf.raw

    def comm_init(self, n_ranks, rank, unique_id):
        buf = C.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES) if unique_id else None
        self._check(self._lib.icpmi_comm_init(self._h, n_ranks, rank, buf))
        self.n_ranks, self.rank = n_ranks, rank

    def comm_init_callbacks(self, n_ranks, rank, allreduce, allgather):
        """allreduce(np_array) / allgather(np_array, per_rank): in-place on a host numpy view."""
        def _ar(_user, buf, count):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(count,)))
                return 0
            except Exception:  # noqa: BLE001 -- must not unwind through C
                import traceback
                traceback.print_exc()
                return 1

        def _ag(_user, buf, per):
            try:
                allgather(np.ctypeslib.as_array(buf, shape=(per * n_ranks,)), per)
                return 0
            except Exception:  # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 1

        self._cb = (ALLREDUCE_FN(_ar), ALLGATHER_FN(_ag))  # keep alive
        self._check(self._lib.icpmi_comm_init_callbacks(self._h, n_ranks, rank, self._cb[0],
                                                        self._cb[1], None))
        self.n_ranks, self.rank = n_ranks, rank

    def comm_finalize(self):
        self._check(self._lib.icpmi_comm_finalize(self._h))
        self.n_ranks, self.rank = 1, 0

    def comm_info(self):
        """icpmi_comm_info (a collective): the communicator's own size and rank, every rank's device and PCI bus id."""
        ci = CommInfo()
        self._check(self._lib.icpmi_comm_info(self._h, C.byref(ci)))
        n = ci.n_ranks
        return {"kind": {0: "none", 1: "rccl", 2: "callbacks"}[ci.kind], "n_ranks": n, "rank": ci.rank,
                "devices": [int(ci.device[r]) for r in range(n)],
                "pci_bus_ids": [bytes(ci.pci_bus_id[r]).split(b"\0")[0].decode() for r in range(n)]}

    def reset_profile(self):
        self._check(self._lib.icpmi_reset_profile(self._h))

    def get_profile(self):
        p = Profile()
        self._check(self._lib.icpmi_get_profile(self._h, C.byref(p)))
        return {f[0]: getattr(p, f[0]) for f in Profile._fields_}

    def nn_reuse_passes(self, cap=1024):
        """Per bounded pass of the last registration (profiling on, all-pairs engine with list reuse): the rows its coarse
        pass listed and the workgroup columns it ran (ceil(rows / rows per workgroup)), as two lists; empty without list reuse or profiling.
        A lean pass (ICPMI_NN_LEAN, get_profile()["nn_lean_passes"]) has no coarse launch: its rows are the rows that wanted a
        list, its columns 0."""
        fn = self._lib.icpmi_debug_nn_reuse
        fn.restype = C.c_int64
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int64]
        rows, blocks = (C.c_uint32 * cap)(), (C.c_uint32 * cap)()
        n = min(int(fn(self._h, rows, blocks, cap)), cap)
        return list(rows[:n]), list(blocks[:n])

    def nn_margin_passes(self, cap=1024):
        """Per bounded pass of the last registration (profiling on, all-pairs engine with the match margin on): the rows
        whose kept match was certified, which the pass neither listed nor scanned; empty where the margin was off."""
        fn = self._lib.icpmi_debug_nn_margin
        fn.restype = C.c_int64
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int64]
        rows = (C.c_uint32 * cap)()
        n = min(int(fn(self._h, rows, cap)), cap)
        return list(rows[:n])

    def debug_loop_rows(self, n):
        """The rows the last registration's last pass matched, as the loop left them: (idx, cur, perm, idx_valid) in the
        loop's internal order of rows -- row r of `cur` is source row perm[r] moved by the pose of that pass, idx[r] its
        match.  `n` must be the registration's row count.  idx_valid is False where the last pass's matches were never
        written to memory (the small-cloud kernel's loop): idx is then all -1 and only cur, perm and the history speak."""
        fn = self._lib.icpmi_debug_loop_rows
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_int64]
        idx, cur, perm = np.empty(n, np.int32), np.empty((n, 3)), np.empty(n, np.uint32)
        rc = fn(self._h, idx.ctypes.data_as(C.POINTER(C.c_int32)), cur.ctypes.data_as(C.POINTER(C.c_double)),
                perm.ctypes.data_as(C.POINTER(C.c_uint32)), n)
        if rc not in (OK, DEBUG_NO_IDX):
            raise IcpError(rc, "icpmi_debug_loop_rows: n is not the last registration's row count")
        return idx, cur, perm, rc == OK
