"""The reference node's whole loop without ROS: SlamNode's timer (slam_viz/src/ros/slam_node.cpp:63-185) over
already-downsampled frames, with registration, loop closure and the pose-graph back end behind it.

    pose_graph_.addPrior(0, identity)                                   :66
    per frame k >= 1 (process_frame, :118-175):
        too few points: repeat the last pose, no factor, no addFrame    :125-130
        ICP against the previous frame, identity if not converged or final_error > 1   :132-142
        addOdometryFactor(k-1, k, delta, final_error)                   :145
        loop_detector_.addFrame(curr, k)                                :159
        every 10 frames after 50: detect(), addLoopClosure(match, query, T) per closure   :160-167
    optimize after a frame that found closures (:112-115) and at the end (:106); on success the track's poses become
    getAllPoses() (:177-185).

The detector uses the node's LoopClosureConfig (:77-81).  By default everything runs through the library on `ctx`;
`align`, `loop_backend` and `pose_graph` replace the three parts (the tests put the CPU oracle and
scripts/pose_graph_ref.py there).  Given a `global_map` (global_map.GlobalMap, or scripts/map_ref.py's restatement),
the run also keeps every frame in it (:71,123), rebuilds the recent clouds after each successful optimize (:187-194)
and at the end the cell set and the published map (build_final_global_map, :196-209, :223-229, :235-238).  With
loop_on_device the detector's database lives on the device as an index over the kept scans (icpmi_loop): the global
map's, or a private store's.  As in the reference, the frame after a too-few-points frame names a pose with no
estimate: its addOdometryFactor raises (ICPMI_ERR_ARG), where the reference throws."""
import numpy as np

from . import loop_closure as lc


class SlamRun:
    def __init__(self):
        self.poses = [np.eye(4)]      # slam_node.cpp:64
        self.factors = []             # ("prior", i, T) / ("odom", i, j, T, fitness) / ("loop", i, j, T), in call order;
        #                               with edge_information also ("odom_info", i, j, T, info) / ("loop_info", i, j, T, info)
        self.closures = []            # LoopClosureResult, in the order found
        self.optimizations = []       # (frame index or "end", ok, stats) per optimize()
        self.recent_world = []        # with a global map: recent_clouds_world_ after each successful optimize
        self.cells = None             # ... and at the end the rebuilt cell set ((n, 2) int32, sorted)
        self.published_map = None     # ... and voxel_downsample(global map, map_voxel)
        self.raster = None            # ... and, with raycast=True, the free / occupied / unknown raster
        self.counts = None            # ... and, with counts=True, the per-cell hit and miss counts
        self.live = None              # ... and, with live=True, the counts kept up to date frame by frame
        self.live_log = []            # ... with (frames_cast, rebuilt) per live_update, in call order
        self.loop_weights = None      # with loop_edge_loss: each closure's weight after the final optimize, if it succeeded
        self.loop_distances = None    # ... and its whitened distance (sigmas)
        self.rejected_closures = []   # with closure_gate: (LoopClosureResult, d2) of every closure the gate kept out
        self.odom_twists = []         # with deskew: the twist each frame was deskewed with
        self.published_map_static = None   # with static_map and a global map: the published map without the dropped rows
        self.static_info = None       # ... and the capi.StaticInfo of that call


def node_loop_config():
    """slam_node.cpp:77-80"""
    return lc.LoopClosureConfig(frame_gap=50, sc_distance_threshold=0.2, icp_fitness_threshold=0.3)


def run_slam(frames, ctx, max_iterations=50, tolerance=1e-6, min_points=1000, pose_graph_config=None,
             align=None, loop_backend=None, pose_graph=None, global_map=None, grid=None, map_voxel=1.0,
             loop_on_device=False, raycast=False, counts=False, live=False, loop_yaw_guess=False, loop_gate=None,
             ground=None, odom_robust=None, loop_robust=None, odom_local_map=None, loop_edge_loss=None,
             edge_information=None, information_floor=(1.0, 10.0), closure_gate=None, deskew=None, deskew_voxel=0.5, odom_gicp=None,
             static_map=None, loop_gicp=None):
    """frames: sequence of N x 3 fp64 clouds (already downsampled).  Returns a SlamRun.  global_map: an object with
    add_frame, recent_clouds and finish (None: no map is built); grid: its occupancy grid config (None: defaults).
    loop_on_device: the detector is loop_closure.StoreLoopClosureDetector over global_map (a global_map.GlobalMap),
    or over a private GlobalMap that keeps every frame; it holds no clouds and gives the same closures.
    raycast: with a global_map, SlamRun.raster = global_map.raycast(poses, grid) after its finish.
    counts: with a global_map, SlamRun.counts = global_map.raycast_counts(poses, grid) after its finish.
    live: with a global_map, global_map.live_update(poses, grid) after each frame's pose is known and after each
    optimize, (frames_cast, rebuilt) of each in SlamRun.live_log; SlamRun.live = the live counts on the final poses.
    loop_yaw_guess: the detector (whichever is built) starts each verification from Scan Context's column shift
    (LoopClosureConfig.yaw_guess; not in the reference node), so a street driven back the other way closes too.
    loop_gate: metres (None: none); the detector's verifications run behind that correspondence-distance gate
    (LoopClosureConfig.max_correspondence_distance; not in the reference node), so a return leg a lane aside closes.
    ground: a ground.GroundConfig (None: none); with a global_map, global_map.set_ground(ground) before the first
    frame, so the cell set, raster, counts and live counts take each frame's OBSTACLE rows as its hits (not in the
    reference node).  Ignored without a global_map.
    static_map: a capi.StaticRule or (min_probability, min_observations) (None: none); with a global_map, after its finish,
    SlamRun.published_map_static, SlamRun.static_info = global_map.finish_static(poses, grid, rule, map_voxel): the
    published map without the rows whose cells the counts outvote (not in the reference node).  The
    recent_world clouds after an optimize stay as they are.  Ignored without a global_map.
    odom_robust: (kind, scale) or (kind, scale, max_distance), kind one of capi.ROBUST_* (None: none); the default
    `align` registers under those row weights (odometry.gpu_align(ctx, robust=...); not in the reference node).  With an
    `align` of the caller's it is refused.
    odom_gicp: (epsilon,) or (epsilon, max_distance) (None: none); the default `align` minimises the plane-to-plane cost
    (odometry.gpu_align(ctx, gicp=...), icpmi_align_gicp; not in the reference node).  Refused with an `align` of the
    caller's, with odom_robust and with odom_local_map (whose registrations have no plane-to-plane form).
    loop_robust: (kind, scale) (None: none); the detector's verifications run under those row weights
    (LoopClosureConfig.robust_kind / robust_scale), behind loop_gate if that is given too.
    loop_gicp: epsilon (None: none); the detector's verifications are plane-to-plane registrations in their small form
    (LoopClosureConfig.gicp_epsilon; not in the reference node), behind loop_gate if that is given too.  Together with
    loop_robust it raises ValueError.
    odom_local_map: a local_map.LocalMapConfig (None: frame-to-frame, as the reference node); each odometry factor's
    delta and final_error come from scan-to-local-map odometry (odometry.LocalMapOdometry; not in the reference node).
    The local map lives in its own odometry frame and is never touched by optimize: the factor is pose_{k-1}^-1 . pose_k
    of that frame, and the track goes on as poses[-1] @ delta.  Combines with odom_robust; with an `align` of the
    caller's it is refused.
    loop_edge_loss: (kind, scale), kind one of capi.PG_LOSS_* (None: none); pose_graph.set_loop_loss(kind, scale) on
    whichever graph is in use, before the prior is added (not in the reference node): the back end prices every loop
    closure under that robust loss and can refuse a false one.  The factor list does not depend on it.
    SlamRun.loop_weights / loop_distances = pose_graph.loop_weights() after the final optimize when that succeeded.
    edge_information: sigma in metres (None: off), the residual noise of one point-to-plane pair (not in the reference
    node).  The edge of every good registration -- odometry and loop closure alike -- is then weighted by the
    6 x 6 information capi.information_from_icp makes of that registration's own normal matrix
    (Context.last_normal_matrix) with this sigma and information_floor = (sigma_R, sigma_t), and enters through
    pose_graph.add_odometry_information / add_loop_closure_information: stiff where the scans constrain the pose, soft
    along a corridor.  SlamRun.factors records it as ("odom_info", i, j, T, info) / ("loop_info", i, j, T, info).  A
    registration the node's gate rejects enters as before, the identity under the diagonal model.  The default floor, one
    radian and ten metres, is far looser than any registration and only keeps a degenerate one positive definite.  The
    closures found and their transforms do not depend on it.  Works with odom_robust, loop_gate, loop_robust,
    loop_edge_loss and odom_local_map (whose registration's T is the pose in the odometry frame: the adjoint is taken at
    that T); with an `align` or a `loop_backend` of the caller's it is refused, their normal matrices are not the library's.
    Under weights final_error is a weighted RMS and reads lower than the plain one: the gate `> 1.0` above, the
    detector's fitness threshold and the odometry factors' noise all read that number.
    closure_gate: a bound on d^2, chi-squared with 6 degrees of freedom, the caller's number (None: no gate, the run is
    call for call what it was; not in the reference node).  When detect() yields closures at frame k the
    graph is optimised once, logged in SlamRun.optimizations under the tag ("gate", k), and every closure of that
    detect() is judged against that one state: d^2 = pose_graph.closure_distance(match, query, transform, Sigma_edge),
    Sigma_edge the loop factor's own noise (the configured loop sigmas squared, or the inverse of the edge's
    information matrix under edge_information).  Closures with d^2 <= closure_gate are added as without a gate; the
    others go to SlamRun.rejected_closures as (closure, d^2) and never enter the graph.
    deskew: a deskew.DeskewConfig (None: none; not in the reference node).  The frames are then RAW sweeps,
    each `points` or `(points, times)`: before anything else sees it, a frame is deskewed (icpmi_deskew) with the twist of
    the previous odometry delta (deskew.twist_from_delta; a zero twist for frames 0 and 1, and after a frame of too few
    points) and filtered with deskew_voxel (icpmi_voxel_downsample).  What is kept, registered, mapped and searched for
    closures is that scan; SlamRun.odom_twists holds the twists used."""
    if loop_on_device and loop_backend is not None:
        raise ValueError("loop_backend and loop_on_device=True both choose the detector")
    if align is not None and odom_robust is not None:
        raise ValueError("odom_robust configures the default align; pass a robust align of your own instead")
    if loop_gicp is not None and loop_robust is not None:
        raise ValueError("loop_gicp and loop_robust exclude each other: the plane-to-plane rows carry no robust weights")
    if odom_gicp is not None and (align is not None or odom_robust is not None or odom_local_map is not None):
        raise ValueError("odom_gicp configures the default align; it does not combine with an align of the caller's, "
                         "odom_robust or odom_local_map")
    if edge_information is not None and (align is not None or loop_backend is not None):
        raise ValueError("edge_information reads the library's own normal matrices; it does not combine with an align or "
                         "a loop_backend of the caller's")
    info_args = None
    if edge_information is not None:
        info_args = (float(edge_information), float(information_floor[0]), float(information_floor[1]))
    run = SlamRun()
    if align is not None and odom_local_map is not None:
        raise ValueError("odom_local_map replaces the default align; it does not combine with an align of your own")
    local_odo = None
    if odom_local_map is not None:
        from .odometry import LocalMapOdometry
        local_odo = LocalMapOdometry(ctx, odom_local_map, max_iterations, tolerance, min_points, robust=odom_robust)
        run.odom_weight_sums = []                                    # under odom_robust: per registration
    elif align is None:
        from .odometry import gpu_align
        align = gpu_align(ctx, robust=odom_robust, gicp=odom_gicp)
    if loop_backend is None and not loop_on_device:
        loop_backend = lc.GpuBackend(ctx)
    if pose_graph is None:
        from .pose_graph import PoseGraph
        pose_graph = PoseGraph(ctx, pose_graph_config)
    if loop_edge_loss is not None:
        pose_graph.set_loop_loss(int(loop_edge_loss[0]), float(loop_edge_loss[1]))
    if ground is not None and global_map is not None:
        global_map.set_ground(ground)
    store = None                                                     # (the store the device detector indexes)
    loop_config = node_loop_config()
    loop_config.yaw_guess = bool(loop_yaw_guess)
    if loop_gate is not None:
        loop_config.max_correspondence_distance = float(loop_gate)
    if loop_robust is not None:
        loop_config.robust_kind, loop_config.robust_scale = int(loop_robust[0]), float(loop_robust[1])
    if loop_gicp is not None:
        loop_config.gicp_epsilon = float(loop_gicp)
    if info_args is not None:
        loop_config.information_sigma, loop_config.information_floor = info_args[0], info_args[1:]
    if loop_on_device:
        from .global_map import GlobalMap
        store = global_map if global_map is not None else GlobalMap(ctx)
        detector = lc.StoreLoopClosureDetector(ctx, store, loop_config)
    else:
        detector = lc.LoopClosureDetector(loop_backend, loop_config)

    def keep(cloud):                                                 # downsampled_clouds_.push_back, :71,123
        """-> the store index of the frame just kept (None without a store)"""
        if global_map is not None:
            global_map.add_frame(cloud)
        elif store is not None:
            store.add_frame(cloud)
        return store.size()[0] - 1 if store is not None else None

    def add(kind, *args):
        run.factors.append((kind,) + args)
        if kind == "prior":
            pose_graph.add_prior(*args)
        elif kind == "odom":
            pose_graph.add_odometry_factor(*args)
        elif kind == "odom_info":
            pose_graph.add_odometry_information(*args)
        elif kind == "loop_info":
            pose_graph.add_loop_closure_information(*args)
        else:
            pose_graph.add_loop_closure(*args)

    def live_update():                                               # update_occupancy_grid's place, :152
        if live and global_map is not None:
            info = global_map.live_update(run.poses, grid)
            run.live_log.append((info.frames_cast, info.rebuilt))

    def optimize(tag):                                               # run_pose_graph_optimization, :177-185
        ok = pose_graph.optimize()
        run.optimizations.append((tag, ok, pose_graph.stats))
        if ok:
            run.poses = [np.asarray(p) for p in pose_graph.get_all_poses()]
            if global_map is not None:                               # rebuild_recent_clouds, :182,187-194
                run.recent_world.append(global_map.recent_clouds(run.poses))
        live_update()

    def gate(found, k):
        """-> the closures of one detect() that pass closure_gate, all judged against one optimised state"""
        optimize(("gate", k))
        if not run.optimizations[-1][1]:
            raise RuntimeError("closure_gate: the graph could not be optimised at frame %d" % k)
        cfg = pose_graph.config
        sigma_loop = np.diag([cfg.loop_rotation_sigma ** 2] * 3 + [cfg.loop_translation_sigma ** 2] * 3)
        passed = []
        for c in found:
            edge = np.linalg.inv(np.asarray(c.information, dtype=np.float64)) if info_args is not None else sigma_loop
            d2 = pose_graph.closure_distance(c.match_frame, c.query_frame, np.asarray(c.transform, dtype=np.float64), edge)
            if d2 <= closure_gate:
                passed.append(c)
            else:
                run.rejected_closures.append((c, d2))
        return passed

    last_delta = [None]                                              # the odometry delta the next frame is deskewed with

    def scan(frame):
        if deskew is None:
            return np.ascontiguousarray(frame, dtype=np.float64)
        from . import deskew as dk
        rows, twist = dk.deskew_frame(ctx, frame, deskew, last_delta[0])
        run.odom_twists.append(twist)
        return np.ascontiguousarray(ctx.voxel_downsample(rows, deskew_voxel), dtype=np.float64)

    add("prior", 0, np.eye(4))                                       # :66
    frames = list(frames)
    prev = scan(frames[0])                                           # :69-72
    keep(prev)                                                       # :71
    if local_odo is not None:
        local_odo.push(prev)
    live_update()
    for k in range(1, len(frames)):
        curr = scan(frames[k])
        pending = False
        kept = keep(curr)                                            # :123
        if curr.shape[0] < min_points:                               # :125-130
            run.poses.append(run.poses[-1].copy())
            prev = curr
            last_delta[0] = np.eye(4)
            if local_odo is not None:
                local_odo.push(curr)
            live_update()
            continue
        if local_odo is not None:                                    # scan-to-local-map: the gate keeps the guess
            delta, r, bad = local_odo.push(curr)
            if odom_robust is not None:
                run.odom_weight_sums.append(r.weight_sum)
        else:
            r = align(curr, prev, max_iterations, tolerance)         # :132-138
            bad = (not r.converged) or r.final_error > 1.0           # :139-140
            delta = np.eye(4) if bad else np.asarray(r.transformation, dtype=np.float64)
        run.poses.append(run.poses[-1] @ delta)                      # :142-143
        last_delta[0] = delta
        if info_args is not None and not bad:                        # the registration just run, at its own T
            from . import capi
            nm = ctx.last_normal_matrix()
            add("odom_info", len(run.poses) - 2, len(run.poses) - 1, delta,
                capi.information_from_icp(nm.JtJ, nm.T, *info_args))
        else:
            add("odom", len(run.poses) - 2, len(run.poses) - 1, delta, float(r.final_error))   # :145
        prev = curr                                                  # :151
        live_update()
        detector.add_frame(kept if loop_on_device else curr, k)      # :159
        if k % 10 == 0 and k > 50:                                   # :160
            found = list(detector.detect())                          # :161-166
            if closure_gate is not None and found:
                found = gate(found, k)
            for c in found:
                if info_args is not None:
                    add("loop_info", c.match_frame, c.query_frame, np.asarray(c.transform, dtype=np.float64), c.information)
                else:
                    add("loop", c.match_frame, c.query_frame, np.asarray(c.transform, dtype=np.float64))
                run.closures.append(c)
                pending = True
        if pending:                                                  # :112-115
            optimize(k)
    optimize("end")                                                  # :103-106
    if loop_edge_loss is not None and run.optimizations[-1][1]:
        run.loop_weights, run.loop_distances = pose_graph.loop_weights()
    if global_map is not None:                                       # build_final_global_map, :107,196-209
        run.cells, run.published_map = global_map.finish(run.poses, grid, map_voxel)
        if raycast:
            run.raster = global_map.raycast(run.poses, grid)
        if counts:
            run.counts = global_map.raycast_counts(run.poses, grid)
        if live:
            live_update()
            run.live = global_map.live_counts()[0]
        if static_map is not None:
            run.published_map_static, run.static_info = global_map.finish_static(run.poses, grid, static_map, map_voxel)
    if local_odo is not None:
        local_odo.close()
    if loop_on_device:                                               # the detector (and a private store) go now
        detector.close()
        if global_map is None:
            store.close()
    return run
