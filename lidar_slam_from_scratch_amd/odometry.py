"""Frame-to-frame odometry driver: `SlamNode::process_frame` minus ROS
(slam_viz/src/ros/slam_node.cpp:118-157), the primary caller of the ICP hot path.

    curr = voxel_downsample(load(frame))                      :121-122  (caller supplies clouds)
    if curr.rows() < min_points: repeat last pose; prev = curr :125-130
    result = icp_point_to_plane(source=curr, target=prev, cfg) :132-138
    delta = identity if (!converged || final_error > 1.0)      :139-140
    new_pose = poses.back() * delta                            :142
    prev = curr                                                :152

`align` is any callable (source, target, max_iterations, tolerance) -> object with
.transformation (4x4), .converged, .final_error, .num_iterations -- the HIP library in the
product, the oracle in the parity tests.
"""
import time

import numpy as np


class OdometryTrack:
    def __init__(self):
        self.poses = [np.eye(4)]          # slam_node.cpp:63-64: pose 0 = identity
        self.deltas = []
        self.final_errors = []
        self.iterations = []
        self.converged = []
        self.gated = []                   # True where the identity fallback was taken
        self.frame_ms = []

    def positions(self):
        return np.array([p[:3, 3] for p in self.poses])


def run_odometry(frames, align, max_iterations=50, tolerance=1e-6, min_points=1000):
    """frames: iterable of N x 3 fp64 clouds in the sensor frame (already downsampled)."""
    track = OdometryTrack()
    prev = None
    for k, curr in enumerate(frames):
        curr = np.ascontiguousarray(curr, dtype=np.float64)
        if k == 0:
            prev = curr                    # slam_node.cpp:69-72
            continue
        t0 = time.perf_counter()
        if curr.shape[0] < min_points:     # slam_node.cpp:125-130
            track.poses.append(track.poses[-1].copy())
            track.deltas.append(np.eye(4))
            track.final_errors.append(float("nan"))
            track.iterations.append(0)
            track.converged.append(False)
            track.gated.append(True)
            prev = curr
            track.frame_ms.append(1e3 * (time.perf_counter() - t0))
            continue
        r = align(curr, prev, max_iterations, tolerance)
        bad = (not r.converged) or r.final_error > 1.0       # slam_node.cpp:139-140
        delta = np.eye(4) if bad else np.asarray(r.transformation, dtype=np.float64)
        track.poses.append(track.poses[-1] @ delta)           # slam_node.cpp:142
        track.deltas.append(delta)
        track.final_errors.append(r.final_error)
        track.iterations.append(r.num_iterations)
        track.converged.append(bool(r.converged))
        track.gated.append(bool(bad))
        prev = curr                                           # slam_node.cpp:152
        track.frame_ms.append(1e3 * (time.perf_counter() - t0))
    return track


def gpu_align(ctx, *, robust=None, gicp=None):
    """Adapter: capi.Context -> the `align` callable above.  robust: a capi.Robust, or (kind, scale[, max_distance]) --
    the registrations run under those row weights (icpmi_align_robust; None: none) and their results carry `weight_sum`
    and `pairs`.  final_error is then the WEIGHTED RMS, which reads lower than the plain one against the caller's
    `> 1.0`.  gicp: a capi.Gicp, or (epsilon[, max_distance[, small]]) -- the registrations minimise the plane-to-plane cost
    (icpmi_align_gicp; None: point-to-plane) and their results carry `pairs`; with `small` (capi.GICP_FORM_SMALL) a pass
    is one kernel at the small-cloud kernel's sizes, to rounding the general path's result; not together with `robust`
    (ValueError)."""
    from . import capi
    if robust is not None and gicp is not None:
        raise ValueError("robust= and gicp= exclude each other: the plane-to-plane rows carry no robust weights")

    class _R:
        pass

    def align(source, target, max_iterations, tolerance):
        cfg = capi.Context.make_config(max_iterations=max_iterations, tolerance=tolerance)
        r = _R()
        if gicp is not None:
            res, _hist, info = ctx.align_gicp(source, target, cfg, gicp)
            r.pairs = int(info.pairs)
        elif robust is None:
            res, _hist = ctx.align(source, target, cfg)
        else:
            res, _hist, info = ctx.align_robust(source, target, cfg, robust)
            r.weight_sum, r.pairs = float(info.weight_sum), int(info.pairs)
        r.transformation = np.array(res.transformation[:]).reshape(4, 4)
        r.converged = bool(res.converged)
        r.final_error = res.final_error
        r.num_iterations = res.num_iterations
        return r

    return align


def run_odometry_device(raw_frames, ctx, voxel=0.5, max_iterations=50, tolerance=1e-6, min_points=1000, deskew=None,
                        on_frame=None):
    """The same loop with the clouds resident in HBM: each RAW scan is
    uploaded once, voxel-filtered on the device (slam_node.cpp:122 -> icpmi_voxel_downsample_device)
    and registered against the previous filtered scan, which never left the device
    (slam_node.cpp:132-133,152: the target of frame t+1 is the source of frame t).
    torch is used for device memory only.
    deskew: a deskew.DeskewConfig (None: none) -- a frame is then `points` or `(points, times)`, and before it is
    filtered it is deskewed in place on the device (icpmi_deskew_device) with the twist of the previous frame's delta
    (deskew.twist_from_delta; a zero twist while there is none); track.twists holds the twists used.
    on_frame(k, twist or None, raw rows as filtered (host copy), filtered scan (host copy), result or None): called when
    frame k is done -- for tests; it costs two copies per frame."""
    import torch
    from . import capi
    from . import deskew as dk
    track = OdometryTrack()
    track.twists = []
    prev = None       # (tensor, rows)
    cfg = capi.Context.make_config(max_iterations=max_iterations, tolerance=tolerance)

    def report(k, twist, d_raw, d_cur, n, res):
        if on_frame:
            on_frame(k, twist, d_raw.cpu().numpy(), d_cur[:n].cpu().numpy(), res)

    for k, raw in enumerate(raw_frames):
        t0 = time.perf_counter()
        twist = None
        if deskew is not None:
            raw, times = dk.split_frame(raw)
        d_raw = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float64)).cuda()
        if deskew is not None:
            twist = dk.frame_twist(track.deltas[-1] if track.deltas else None)
            track.twists.append(twist)
            d_times = None if times is None else torch.from_numpy(np.ascontiguousarray(times, dtype=np.float64)).cuda()
            if d_raw.shape[0]:
                ctx.deskew_device(d_raw.data_ptr(), None if d_times is None else d_times.data_ptr(), d_raw.shape[0],
                                  deskew.with_twist(twist).to_c(times is not None), d_raw.data_ptr())
        d_cur = torch.empty_like(d_raw)
        n = ctx.voxel_downsample_device(d_raw.data_ptr(), d_raw.shape[0], voxel, d_cur.data_ptr(), d_raw.shape[0])
        if k == 0:
            prev = (d_cur, n)              # slam_node.cpp:69-72
            report(k, twist, d_raw, d_cur, n, None)
            continue
        if n < min_points:                 # slam_node.cpp:125-130
            track.poses.append(track.poses[-1].copy())
            track.deltas.append(np.eye(4))
            track.final_errors.append(float("nan"))
            track.iterations.append(0)
            track.converged.append(False)
            track.gated.append(True)
            prev = (d_cur, n)
            track.frame_ms.append(1e3 * (time.perf_counter() - t0))
            report(k, twist, d_raw, d_cur, n, None)
            continue
        res, _hist = ctx.align_device(d_cur.data_ptr(), n, prev[0].data_ptr(), prev[1], cfg)
        res.error_history = _hist
        bad = (not res.converged) or res.final_error > 1.0   # slam_node.cpp:139-140
        delta = np.eye(4) if bad else np.array(res.transformation[:]).reshape(4, 4)
        track.poses.append(track.poses[-1] @ delta)           # slam_node.cpp:142
        track.deltas.append(delta)
        track.final_errors.append(res.final_error)
        track.iterations.append(res.num_iterations)
        track.converged.append(bool(res.converged))
        track.gated.append(bool(bad))
        prev = (d_cur, n)                                     # slam_node.cpp:152
        track.frame_ms.append(1e3 * (time.perf_counter() - t0))
        report(k, twist, d_raw, d_cur, n, res)
    return track


def run_odometry_stream(paths, ctx, voxel=0.5, max_iterations=50, tolerance=1e-6, min_points=1000, grid=None,
                        want_world=False, prefetch=True, robust=None):
    """The same loop over frame FILES with everything but the file read on the device: one
    `icpmi_stream_push_file` per frame does slam_node.cpp:121-152 -- the scan goes from disk through
    pinned memory to HBM (`.bin`: float32 records, widened there), voxel filter, min-points guard,
    registration against the previous filtered scan that stayed resident -- and this function
    applies the reference's gate and pose update (slam_node.cpp:139-142).  With `grid` (a
    capi.GridConfig) every frame also gets the map side (slam_node.cpp:147-153, `icpmi_stream_map_update`):
    world points of the resident scan (copied out only with `want_world`) and the occupancy insert;
    track.cells then holds the size of the cell set after each frame.  With `prefetch` the next
    frame's file is read by the library's worker thread while this frame runs
    (`icpmi_stream_prefetch_file`).  robust: a capi.Robust, or (kind, scale[, max_distance]) -- every push registers
    under those row weights (icpmi_stream_set_robust; None: none, and a rule set earlier is cleared); track.weight_sums
    then holds each registration's weight sum.  No torch in here."""
    from . import capi
    track = OdometryTrack()
    track.cells = []
    track.weight_sums = []
    cfg = capi.Context.make_config(max_iterations=max_iterations, tolerance=tolerance)
    ctx.stream_reset()
    ctx.stream_set_robust(robust)
    if grid is not None:
        ctx.occupancy_clear()

    def map_side(n_rows):
        if grid is not None:                                      # slam_node.cpp:147-153
            _w, n_cells = ctx.stream_map_update(track.poses[-1], grid, want_world=want_world, n_rows=n_rows)
            track.cells.append(n_cells)

    paths = list(paths)
    for k, path in enumerate(paths):
        t0 = time.perf_counter()
        if prefetch and k + 1 < len(paths):
            ctx.stream_prefetch_file(paths[k + 1])                # read beside this frame's work
        res, _hist, info = ctx.stream_push_file(path, voxel, min_points, cfg)
        if info.status == capi.STREAM_FIRST_FRAME:                # slam_node.cpp:69-72: kept, not inserted into the grid
            continue
        if info.status == capi.STREAM_TOO_FEW_POINTS:            # slam_node.cpp:125-130
            track.poses.append(track.poses[-1].copy())
            track.deltas.append(np.eye(4))
            track.final_errors.append(float("nan"))
            track.iterations.append(0)
            track.converged.append(False)
            track.gated.append(True)
            track.frame_ms.append(1e3 * (time.perf_counter() - t0))   # (the reference returns before its map update here)
            continue
        bad = (not res.converged) or res.final_error > 1.0        # slam_node.cpp:139-140
        delta = np.eye(4) if bad else np.array(res.transformation[:]).reshape(4, 4)
        track.poses.append(track.poses[-1] @ delta)                # slam_node.cpp:142
        track.deltas.append(delta)
        track.final_errors.append(res.final_error)
        track.iterations.append(res.num_iterations)
        track.converged.append(bool(res.converged))
        track.gated.append(bool(bad))
        if robust is not None:
            track.weight_sums.append(float(ctx.stream_last_robust().weight_sum))
        map_side(info.n_filtered)
        track.frame_ms.append(1e3 * (time.perf_counter() - t0))
    return track


def _rigid_inverse(T):
    """(R^T, -R^T t)"""
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


class LocalMapOdometry:
    """Scan-to-local-map odometry, one frame at a time (not in the reference node): each scan is registered against a
    sliding voxel map of the recent scans (local_map.LocalMap) from a constant-velocity guess, and then added to it under
    the pose found.  The map lives in the odometry's own frame (pose 0 = identity).

        frame 0                pose = I; add(frame, I)
        too few points         the pose repeats, nothing is added, the remembered delta becomes I
        otherwise              guess = pose_prev . delta_prev (pose_prev alone without the motion model)
                               r = register(frame, guess); the node's gate (!converged || final_error > 1) keeps the guess
                               delta = pose_prev^-1 . pose; add(frame, pose) ALWAYS -- a map that skips a gated frame
                               stalls for good

    push(frame) -> None for frame 0, else (delta, result, gated) with result None for a frame of too few points;
    result has the fields of run_odometry's `align` results, .guess, .error_history, and .weight_sum / .pairs under a
    robust rule."""

    def __init__(self, ctx, config=None, max_iterations=50, tolerance=1e-6, min_points=1000, motion_model=True, robust=None,
                 deskew=None, voxel=0.5):
        """deskew: a deskew.DeskewConfig (None: none, and frames are taken as they come, already downsampled) -- a frame
        is then a RAW sweep, `points` or `(points, times)`: it is deskewed (icpmi_deskew) with the twist of the previous
        frame's delta (deskew.twist_from_delta; a zero twist for frames 0 and 1), filtered with `voxel`
        (icpmi_voxel_downsample) and only then registered and added.  self.twist: the one last used."""
        from .local_map import LocalMap
        self.ctx, self.map = ctx, LocalMap(ctx, config)
        self.max_iterations, self.tolerance, self.min_points = max_iterations, tolerance, min_points
        self.motion_model, self.robust = motion_model, robust
        self.pose, self.delta, self.frames = np.eye(4), np.eye(4), 0
        self.deskew, self.voxel, self.twist = deskew, voxel, None

    def close(self):
        self.map.close()

    def push(self, frame):
        from . import capi

        class _R:
            pass

        if self.deskew is not None:
            from . import deskew as dk
            rows, self.twist = dk.deskew_frame(self.ctx, frame, self.deskew, self.delta if self.frames >= 2 else None)
            frame = self.ctx.voxel_downsample(rows, self.voxel)
        curr = np.ascontiguousarray(frame, dtype=np.float64)
        self.frames += 1
        if self.frames == 1:
            self.map.add(curr, self.pose)
            return None
        if curr.shape[0] < self.min_points:
            self.delta = np.eye(4)
            return self.delta, None, True
        guess = self.pose @ self.delta if self.motion_model else self.pose.copy()
        cfg = capi.Context.make_config(max_iterations=self.max_iterations, tolerance=self.tolerance, initial_transform=guess)
        r = _R()
        if self.robust is None:
            res, hist = self.map.register(curr, cfg)
        else:
            res, hist, info = self.map.register_robust(curr, cfg, self.robust)
            r.weight_sum, r.pairs = float(info.weight_sum), int(info.pairs)
        r.guess, r.error_history = guess, hist
        r.transformation = np.array(res.transformation[:]).reshape(4, 4)
        r.converged, r.final_error, r.num_iterations = bool(res.converged), res.final_error, res.num_iterations
        bad = (not r.converged) or r.final_error > 1.0
        pose = guess if bad else r.transformation
        self.delta = _rigid_inverse(self.pose) @ pose
        self.pose = pose
        self.map.add(curr, pose)
        return self.delta, r, bool(bad)


def run_odometry_local_map(frames, ctx, config=None, max_iterations=50, tolerance=1e-6, min_points=1000, motion_model=True,
                           robust=None, on_frame=None, deskew=None, voxel=0.5):
    """Scan-to-local-map odometry over already-downsampled frames (LocalMapOdometry) -> OdometryTrack; track.deltas are
    pose_{k-1}^-1 . pose_k, track.map_rows the table's size after each frame, and under a robust rule (a capi.Robust, or
    (kind, scale[, max_distance])) track.weight_sums each registration's weight sum.  config: a local_map.LocalMapConfig;
    its max_range must cover the sensor's range.  on_frame(k, local map, result or None): called after frame k is done.
    deskew: a deskew.DeskewConfig -- the frames are then RAW sweeps, deskewed and filtered with `voxel` first (see
    LocalMapOdometry); track.twists holds the twists used."""
    odo = LocalMapOdometry(ctx, config, max_iterations, tolerance, min_points, motion_model, robust, deskew, voxel)
    track = OdometryTrack()
    track.map_rows = []
    track.weight_sums = []
    track.twists = []
    try:
        for k, curr in enumerate(frames):
            t0 = time.perf_counter()
            out = odo.push(curr)
            if deskew is not None:
                track.twists.append(odo.twist)
            track.map_rows.append(odo.map.size())
            if out is not None:
                delta, r, bad = out
                track.poses.append(odo.pose.copy())
                track.deltas.append(delta)
                track.final_errors.append(r.final_error if r is not None else float("nan"))
                track.iterations.append(r.num_iterations if r is not None else 0)
                track.converged.append(bool(r.converged) if r is not None else False)
                track.gated.append(bool(bad))
                if robust is not None and r is not None:
                    track.weight_sums.append(r.weight_sum)
                track.frame_ms.append(1e3 * (time.perf_counter() - t0))
            if on_frame:
                on_frame(k, odo.map, out[1] if out is not None else None)
    finally:
        odo.close()
    return track


def absolute_trajectory_error(track, truth_poses):
    """RMS translation error against ground-truth poses expressed relative to frame 0."""
    t0_inv = np.linalg.inv(truth_poses[0])
    err = [np.linalg.norm((t0_inv @ T)[:3, 3] - P[:3, 3]) for T, P in zip(truth_poses, track.poses)]
    return float(np.sqrt(np.mean(np.square(err))))
