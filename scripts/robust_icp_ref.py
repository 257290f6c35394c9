"""scripts/robust_icp_ref.py -- the CPU restatement of point-to-plane ICP under robust row weights that
tests/test_robust_reference.py and tests/test_gpu_robust.py hold the library to.

The reference gives every source row the same say in the normal equations (icp.hpp:89-144).  Here, per pass, for row i
with nearest target j (`found`: the row has a neighbour), in unfused fp64 and in this order:

    e  = q_j - p_i
    d2 = (e0*e0 + e1*e1) + e2*e2
    b  = (e0*n0 + e1*n1) + e2*n2          (icp.hpp:116)

Gate: the row is kept iff found && d2 <= g2, with g2 = max_distance*max_distance when a gate is given and g2 = DBL_MAX
when max_distance == 0; a NaN or infinite row is then still dropped.
Weight of a kept row, a = fabs(b):
    HUBER           w = a <= k ? 1.0 : k / a
    GEMAN_MCCLURE   s = k*k (formed once), t = s + b*b, r = s / t, w = r*r
Sums over the kept rows, wJ[r] = w*J[r]: columns 0..20 add wJ[r]*J[c], columns 21..26 add wJ[r]*b, column 27 adds
(w*b)*b, column 28 adds w, column 29 adds 1.0 (the pairs).  A dropped row adds nothing.  With w == 1.0 every product is
the unweighted one: a Huber scale above every |b| gives gated_icp_ref.gated_icp's bits, and with no gate the oracle's.
Error: sqrt(sums[27] / sums[28]), the weighted RMS; it feeds final_error, the history and both stopping tests.  A pass
with !(sums[28] > 0) ends the call as gated_icp's pass without pairs does.  Step, composition, post-loop entry and the
history invariants are icp.hpp:157-258 as oracle/icp_oracle.c restates it.

The sums are formed in numpy, row after row in index order (a cumulative sum, not numpy's pairwise one), which is the
order of oracle/icp_oracle.c's loop: that is what makes the w == 1.0 case the oracle's to the bit.

    robust_icp(source, target, kind, scale, max_distance=0.0, ...)
    RobustOracleBackend          robust_icp behind loop_yaw_ref.YawLoopClosureDetector's backend interface
    cars_pair()                  synth.c2_lidar_pair() with five parked-car boxes that move 1.5 m between the scans
    drive_frames(n)              frames 0..n-1 of the default drive and their true poses
    odometry_ate(frames, align)  frame-to-frame odometry with the caller's identity gate -> (ATE rms, end error, passes)

A redescending weight needs a start inside its basin: Geman-McClure at 0.1 m locks onto the identity when the start is
a metre off (C2 pair: 0.97 m from truth), at 0.3 m it does about as well as Huber at 0.1 m.  That is the algorithm."""
import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gated_icp_ref as gr  # noqa: E402
import loop_yaw_ref as yr  # noqa: E402

DBL_MAX = sys.float_info.max
HUBER, GEMAN_MCCLURE = 1, 2   # ICPMI_ROBUST_*
HUBER_SCALE, GM_SCALE = 0.1, 0.3


def weights(kind, scale, b):
    """the contract's weight of every residual in b"""
    if kind == HUBER:
        a = np.fabs(b)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(a <= scale, 1.0, scale / a)
    if kind != GEMAN_MCCLURE:
        raise ValueError("kind must be HUBER or GEMAN_MCCLURE")
    s = scale * scale
    t = s + b * b
    r = s / t
    return r * r


def weighted_sums(p, q, n, kind, scale):
    """the 30 columns over the rows given (all kept), each added row after row in index order"""
    J = np.empty((p.shape[0], 6))
    J[:, 0] = p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1]                  # p x n, icp.hpp:105
    J[:, 1] = p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2]
    J[:, 2] = p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0]
    J[:, 3:] = n
    e = q - p
    b = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]  # icp.hpp:116
    w = weights(kind, scale, b)
    wJ = w[:, None] * J
    cols = np.empty((p.shape[0], 30))
    o = 0
    for r in range(6):
        for c in range(r, 6):
            cols[:, o] = wJ[:, r] * J[:, c]
            o += 1
    for r in range(6):
        cols[:, 21 + r] = wJ[:, r] * b
    cols[:, 27] = (w * b) * b
    cols[:, 28] = w
    cols[:, 29] = 1.0
    return np.cumsum(cols, axis=0)[-1]                               # (sequential, unlike np.sum)


class RobustResult:
    """ICPResult's fields (types.hpp:155-164) + weight_sum and pairs (of the pass that produced final_error) +
    stop_margin (the smallest | |prev - error| - tolerance | over the loop's passes: how far the iteration count is from
    hanging on rounding) + gate_margin (the smallest |d2 - g2| over every row of every pass; inf without a gate)"""


def robust_icp(source, target, kind, scale, max_distance=0.0, max_iterations=50, tolerance=1e-6, min_error=1e-9,
               initial_transform=None, orc=None, normals=None, tree=None):
    """-> RobustResult.  normals / tree: the target's, if the caller has them already."""
    if orc is None:
        from oracle import oracle as orc
    if kind not in (HUBER, GEMAN_MCCLURE):
        raise ValueError("kind must be HUBER or GEMAN_MCCLURE")
    if not (scale > 0.0 and math.isfinite(scale)):
        raise ValueError("scale must be finite and > 0")
    if max_distance != 0.0 and not (max_distance > 0.0 and math.isfinite(max_distance)):
        raise ValueError("max_distance must be 0 or finite and > 0")
    src = np.ascontiguousarray(source, dtype=np.float64)
    tgt = np.ascontiguousarray(target, dtype=np.float64)
    gated = max_distance != 0.0
    g2 = float(max_distance) * float(max_distance) if gated else DBL_MAX
    tree = tree or orc.KDTree(tgt)                                   # icp.hpp:166
    nrm = normals if normals is not None else orc.estimate_normals(tgt, tree, 20)   # :169-171
    T0 = np.eye(4) if initial_transform is None else np.array(initial_transform, dtype=np.float64).reshape(4, 4)
    cur = gr.apply_rt(T0, src)                                       # :174-176
    total = T0.copy()                                                # :178
    prev = DBL_MAX                                                   # :179
    hist, converged = [], False
    gate_margin, stop_margin = math.inf, math.inf

    def one_pass():
        """-> the 30 sums, or None when no row is kept"""
        nonlocal gate_margin
        idx, _ = tree.nearest_batch(cur)
        found = (idx >= 0) & (idx < tgt.shape[0])
        j = np.where(found, idx, 0)
        e = tgt[j] - cur
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            keep = found & (d2 <= g2)                                # (false for a NaN, and for +Inf against DBL_MAX)
            fin = np.isfinite(d2)
            if gated and fin.any():
                gate_margin = min(gate_margin, float(np.min(np.abs(d2[fin] - g2))))
        if not keep.any():
            return None
        return weighted_sums(cur[keep], tgt[j[keep]], nrm[j[keep]], kind, scale)

    no_pairs, sums = False, None
    for _ in range(int(max_iterations)):                             # :181
        sums = one_pass()
        if sums is None or not (sums[28] > 0.0):                     # no pairs: a break without convergence
            hist += [math.inf, math.inf]
            no_pairs = True
            break
        error = math.sqrt(sums[27] / sums[28])
        hist.append(error)                                           # :207
        stop_margin = min(stop_margin, abs(abs(prev - error) - tolerance))
        if error < min_error or abs(prev - error) < tolerance:       # :210-217
            converged = True
            break
        delta = orc.solve_from_sums(np.ascontiguousarray(sums[:28]))  # :220
        cur = gr.apply_rt(delta, cur)                                # :225-226
        total = gr.mul44(delta, total)                               # :229
        prev = error                                                 # :231
    if not no_pairs:                                                 # :235-252
        sums = one_pass()
        ok = sums is not None and sums[28] > 0.0
        hist.append(math.sqrt(sums[27] / sums[28]) if ok else math.inf)
    r = RobustResult()
    r.transformation = total
    r.converged = converged
    r.error_history = np.array(hist)
    r.num_iterations = len(hist) - 1                                 # :255
    r.final_error = hist[-1]
    r.weight_sum = 0.0 if sums is None else float(sums[28])
    r.pairs = 0 if sums is None else int(sums[29])
    r.stop_margin = stop_margin
    r.gate_margin = gate_margin
    return r


class RobustOracleBackend(yr.OracleBackend):
    """robust_icp behind YawLoopClosureDetector's backend interface.  Every verification is kept in `runs`, in call
    order; run_of(closure) is the one a closure came from (the detector hands its transform array on as it is)."""

    def __init__(self, kind, scale, max_distance=0.0, orc=None):
        super().__init__(orc)
        self.kind, self.scale, self.max_distance = int(kind), float(scale), float(max_distance)
        self.runs = []
        self._normals = {}                                            # per target (by identity): (tree, normals)

    def align(self, s, t, max_iterations, tolerance, *, initial_transform=None):
        key = id(t)
        if key not in self._normals:
            tree = self.orc.KDTree(t)
            self._normals[key] = (t, tree, self.orc.estimate_normals(t, tree, 20))
        _, tree, nrm = self._normals[key]
        r = robust_icp(s, t, self.kind, self.scale, self.max_distance, max_iterations, tolerance, 1e-9,
                       initial_transform, orc=self.orc, normals=nrm, tree=tree)
        self.iterations.append(r.num_iterations)
        self.runs.append(r)
        return r

    def run_of(self, closure):
        for r in self.runs:
            if r.transformation is closure.transform:
                return r
        raise KeyError("not a closure of this backend")

    def min_margins(self):
        """-> (stopping margin, gate margin) over every verification"""
        return (min((r.stop_margin for r in self.runs), default=math.inf),
                min((r.gate_margin for r in self.runs), default=math.inf))


# The "cars": five boxes of 4.5 x 1.8 x 1.5 m standing on the road (z from -1.73), on either side of the sensor's lane
# around where the C2 pair is taken (x = -40, -39); each is 1.5 m further along x in the second scan.
CAR_CENTRES = ((-33.0, 2.6), (-29.0, -2.7), (-46.0, 2.5), (-24.0, 2.8), (-50.0, -2.6))
CAR_HALF = (2.25, 0.9)
CAR_HEIGHT = 1.5
CAR_MOVE = 1.5


def _cars(dx):
    return [(np.array([cx + dx - CAR_HALF[0], cy - CAR_HALF[1], -1.73]),
             np.array([cx + dx + CAR_HALF[0], cy + CAR_HALF[1], -1.73 + CAR_HEIGHT])) for cx, cy in CAR_CENTRES]


def cars_pair(voxel=0.5, beams=64, azimuths=1800, range_noise=0.01):
    """-> (source, target, truth): synth.c2_lidar_pair() -- frames 1 and 0 of the default drive, same range noise --
    with the five cars in the scene, CAR_MOVE further along x when the source (frame 1) is taken"""
    from lidar_slam_from_scratch_amd import synth
    out = []
    for frame, dx in ((0, 0.0), (1, CAR_MOVE)):
        T = synth.lidar_pose(frame)
        pts = synth._raycast(T[:3, 3], T[:3, :3], synth._scene(3) + _cars(dx), beams=beams, azimuths=azimuths)
        rng = np.random.Generator(np.random.PCG64(1000 + frame))
        r = np.linalg.norm(pts, axis=1, keepdims=True)
        pts = pts * (1.0 + rng.normal(0.0, range_noise, size=r.shape) / np.maximum(r, 1e-9))
        out.append(synth.voxel_centroids(pts, voxel))
    truth = synth.invert_transform(synth.lidar_pose(0)) @ synth.lidar_pose(1)
    return out[1], out[0], truth


def drive_frames(n):
    """-> (frames, poses): synth.lidar_frame(f) and synth.lidar_pose(f) for f in 0..n-1"""
    from lidar_slam_from_scratch_amd import synth
    return [synth.lidar_frame(f) for f in range(n)], [synth.lidar_pose(f) for f in range(n)]


def odometry_ate(frames, poses, align):
    """frame-to-frame odometry (odometry.run_odometry: the caller's identity gate) -> (ATE rms, end error, passes)"""
    from lidar_slam_from_scratch_amd import odometry
    track = odometry.run_odometry(frames, align)
    end = float(np.linalg.norm((np.linalg.inv(poses[0]) @ poses[-1])[:3, 3] - track.poses[-1][:3, 3]))
    return odometry.absolute_trajectory_error(track, poses), end, int(sum(track.iterations))


def oracle_align(orc=None):
    """the oracle as run_odometry's `align`"""
    if orc is None:
        from oracle import oracle as orc
    return lambda s, t, it, tol: orc.icp_point_to_plane(s, t, max_iterations=it, tolerance=tol)


def robust_align(kind, scale, max_distance=0.0, orc=None):
    """robust_icp as run_odometry's `align`"""
    return lambda s, t, it, tol: robust_icp(s, t, kind, scale, max_distance, it, tol, orc=orc)


def truth_error(T, truth):
    from lidar_slam_from_scratch_amd import synth
    return synth.pose_delta(np.asarray(T), truth)[0]


def l12_worst(closures, poses, labels):
    """the largest translation error of a set of L12 closures against the drive's truth"""
    from lidar_slam_from_scratch_amd import synth
    worst = 0.0
    for c in closures:
        dt, _ = synth.pose_delta(c.transform, yr.truth(poses, labels.index(c.query_frame), labels.index(c.match_frame)))
        worst = max(worst, dt)
    return worst


if __name__ == "__main__":
    from oracle import oracle as orc
    from lidar_slam_from_scratch_amd import synth
    for name, (s, t, T) in (("C2 pair", synth.c2_lidar_pair()), ("cars pair", cars_pair())):
        plain = orc.icp_point_to_plane(s, t)
        print("%-10s plain %.4f m, %d iterations" % (name, truth_error(plain.transformation, T), plain.num_iterations))
        for label, kind, k in (("Huber 0.1", HUBER, 0.1), ("GM 0.3", GEMAN_MCCLURE, 0.3), ("GM 0.1", GEMAN_MCCLURE, 0.1)):
            r = robust_icp(s, t, kind, k)
            print("%-10s %-9s %.4f m, %d iterations, weight sum %.3f of %d pairs, stopping margin %.2e"
                  % (name, label, truth_error(r.transformation, T), r.num_iterations, r.weight_sum, r.pairs, r.stop_margin))
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 25
    frames, poses = drive_frames(n)
    print("drive 0..%d plain     ATE rms %.3f m, end %.3f m, %d iterations" % ((n - 1,) + odometry_ate(frames, poses, oracle_align())))
    print("drive 0..%d Huber 0.1 ATE rms %.3f m, end %.3f m, %d iterations"
          % ((n - 1,) + odometry_ate(frames, poses, robust_align(HUBER, HUBER_SCALE))))
    poses12, labels, clouds = gr.l12_scans()
    for name, backend in (("gate 2 m", gr.GatedOracleBackend(gr.L12_GATE)),
                          ("Huber 0.1 + gate 2 m", RobustOracleBackend(HUBER, HUBER_SCALE, gr.L12_GATE))):
        res = gr.run_detector(yr.YawLoopClosureDetector(backend, gr.l12_config()), clouds, labels)
        print("L12 %-21s verifications %d, closures %d, worst %.4f m"
              % (name, len(backend.iterations), len(res), l12_worst(res, poses12, labels)))
