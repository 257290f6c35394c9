"""scripts/gated_icp_ref.py -- the CPU restatement of point-to-plane ICP behind a correspondence-distance gate (DESIGN
7.8) that tests/test_gated_reference.py and tests/test_gpu_gated.py hold the library to.

The reference sums every source row into the normal equations (icp.hpp:89-144).  Here, with g2 = max_distance *
max_distance, a pass keeps row i with nearest target j iff

    e = q_j - p_i;   d2 = (e0 * e0 + e1 * e1) + e2 * e2   (fp64, unfused, this order);   d2 <= g2

and a row with a non-finite coordinate, or without a neighbour, is dropped.  The 28 sums run over the kept rows, the
error is their RMS sqrt(sum b^2 / kept), and everything else is icp.hpp:157-258 as oracle/icp_oracle.c restates it: the
two tests in front of the solve, total = delta * total, the post-loop entry.  A pass that keeps no row ends the call like
a break without convergence, with +Inf as that pass's error and again as the post-loop entry.

    gated_icp(source, target, max_distance, ...)   built from the oracle's primitives: KDTree.nearest_batch,
                                                   estimate_normals, normal_equations on the kept rows, solve_from_sums
    GatedOracleBackend                             gated_icp behind loop_yaw_ref.YawLoopClosureDetector's backend interface
    l12_lateral_drive()                            loop_yaw_ref's R12 with the return leg 1.5 m aside, at y = 1.8

Measured on L12 with frame_gap 50, sc_distance_threshold 0.3 (the drive's descriptor distances reach 0.25),
icp_fitness_threshold 0.3, max_candidates 3: ungated 5 closures of 13 verifications, return scans 100..102 without one;
at 2.0 m 12 closures, every return scan closes, the worst 0.16 m from truth.  A tight gate can chatter: at 1.0 m one
pair of the un-offset R12 runs its 30 iterations without meeting the tolerance, the kept set alternating.  That is the
algorithm; the fixtures use 2.0 m."""
import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import loop_yaw_ref as yr  # noqa: E402

DBL_MAX = sys.float_info.max
L12_CONFIG = dict(frame_gap=50, sc_distance_threshold=0.3, icp_fitness_threshold=0.3, max_candidates=3)
L12_GATE = 2.0


def apply_rt(T, pts):
    """cloud * R^T + t^T row-wise in the oracle's operation order (icp_oracle.c apply_rt)"""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = np.empty_like(pts)
    for r in range(3):
        out[:, r] = ((x * T[r, 0] + y * T[r, 1]) + z * T[r, 2]) + T[r, 3]
    return out


def mul44(A, B):
    """A * B with the inner sums in index order from 0 (icp_oracle.c mul44)"""
    out = np.empty((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += A[i, k] * B[k, j]
            out[i, j] = s
    return out


class GatedResult:
    """ICPResult's fields (types.hpp:155-164) + pairs (rows kept by the pass that produced final_error) + min_margin
    (the smallest |d2 - g2| over every row of every pass: how far the kept sets are from hanging on rounding)"""


def gated_icp(source, target, max_distance, max_iterations=50, tolerance=1e-6, min_error=1e-9, initial_transform=None,
              orc=None, normals=None, tree=None):
    """-> GatedResult.  normals / tree: the target's, if the caller has them already."""
    if orc is None:
        from oracle import oracle as orc
    if not (max_distance > 0.0 and math.isfinite(max_distance)):
        raise ValueError("max_distance must be finite and > 0")
    src = np.ascontiguousarray(source, dtype=np.float64)
    tgt = np.ascontiguousarray(target, dtype=np.float64)
    g2 = float(max_distance) * float(max_distance)
    tree = tree or orc.KDTree(tgt)                                   # icp.hpp:166
    nrm = normals if normals is not None else orc.estimate_normals(tgt, tree, 20)   # :169-171
    T0 = np.eye(4) if initial_transform is None else np.array(initial_transform, dtype=np.float64).reshape(4, 4)
    cur = apply_rt(T0, src)                                          # :174-176
    total = T0.copy()                                                # :178
    prev = DBL_MAX                                                   # :179
    hist, converged, margin = [], False, math.inf

    def one_pass():
        """-> (sums over the kept rows or None, kept count)"""
        nonlocal margin
        idx, _ = tree.nearest_batch(cur)
        found = (idx >= 0) & (idx < tgt.shape[0])
        j = np.where(found, idx, 0)
        e = tgt[j] - cur
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            keep = found & (d2 <= g2)                                # (false for a NaN)
            fin = np.isfinite(d2)
            if fin.any():
                margin = min(margin, float(np.min(np.abs(d2[fin] - g2))))
        count = int(keep.sum())
        if count == 0:
            return None, 0
        return orc.normal_equations(cur[keep], tgt[j[keep]], nrm[j[keep]]), count

    no_pairs, pairs = False, 0
    for _ in range(int(max_iterations)):                             # :181
        sums, pairs = one_pass()
        if sums is None:                                             # no pairs: a break without convergence
            hist += [math.inf, math.inf]
            no_pairs = True
            break
        error = math.sqrt(sums[27] / pairs)
        hist.append(error)                                           # :207
        if error < min_error or abs(prev - error) < tolerance:       # :210-217
            converged = True
            break
        delta = orc.solve_from_sums(sums)                            # :220
        cur = apply_rt(delta, cur)                                   # :225-226
        total = mul44(delta, total)                                  # :229
        prev = error                                                 # :231
    if not no_pairs:                                                 # :235-252
        sums, pairs = one_pass()
        hist.append(math.inf if sums is None else math.sqrt(sums[27] / pairs))
    r = GatedResult()
    r.transformation = total
    r.converged = converged
    r.error_history = np.array(hist)
    r.num_iterations = len(hist) - 1                                 # :255
    r.final_error = hist[-1]
    r.pairs = pairs
    r.min_margin = margin
    return r


class GatedOracleBackend(yr.OracleBackend):
    """gated_icp behind YawLoopClosureDetector's backend interface.  Every verification is kept in `runs`, in call
    order; run_of(closure) is the one a closure came from (the detector hands its transform array on as it is)."""

    def __init__(self, max_distance, orc=None):
        super().__init__(orc)
        self.max_distance = float(max_distance)
        self.runs = []
        self._normals = {}                                            # per target (by identity): (tree, normals)

    def align(self, s, t, max_iterations, tolerance, *, initial_transform=None):
        key = id(t)
        if key not in self._normals:
            tree = self.orc.KDTree(t)
            self._normals[key] = (t, tree, self.orc.estimate_normals(t, tree, 20))
        _, tree, nrm = self._normals[key]
        r = gated_icp(s, t, self.max_distance, max_iterations, tolerance, 1e-9, initial_transform, orc=self.orc,
                      normals=nrm, tree=tree)
        self.iterations.append(r.num_iterations)
        self.runs.append(r)
        return r

    def run_of(self, closure):
        for r in self.runs:
            if r.transformation is closure.transform:
                return r
        raise KeyError("not a closure of this backend")

    def min_margin(self):
        return min((r.min_margin for r in self.runs), default=math.inf)


def l12_lateral_drive():
    """-> (poses, labels): loop_yaw_ref.r12_reverse_drive() with the six return poses 1.5 m aside (y = 1.8)"""
    out = [yr.pose(-20 + 2 * k, 0.3, 2 * k) for k in range(6)]
    back = [yr.pose(-20 + 2 * k, 1.8, 183 - 1.5 * k) for k in range(5, -1, -1)]
    return out + back, list(range(6)) + list(range(100, 106))


def l12_scans():
    """-> (poses, labels, clouds) of L12"""
    poses, labels = l12_lateral_drive()
    return poses, labels, yr.scans(poses)


L12_PAIRS = ((8, 3), (6, 5))   # (query, match) positions in the drive: 2,925 -> 3,729 and 4,342 -> 4,372 rows


def l12_pair(clouds, query, match, orc=None):
    """-> (source, target, start): an L12 pair with the start its verification has, shift_transform of the pair's shift"""
    if orc is None:
        from oracle import oracle as orc
    _, shift = yr.distance_shift(orc.scan_context(clouds[query]), orc.scan_context(clouds[match]))
    return clouds[query], clouds[match], yr.shift_transform(shift)


def general_pair():
    """-> (source 700 x 3, target 17,000 x 3): every tenth row of a street scan taken 1.5 m aside of, and 2 degrees
    off, a denser scan (0.25 m voxels) thinned to 17,000 rows -- nine splits of 2,048, past the small-cloud kernel"""
    from lidar_slam_from_scratch_amd import synth
    dense = synth.lidar_frame_at(yr.pose(-10, 0.3, 0), 7, voxel=0.25, beams=64, azimuths=1800)
    rows = np.sort(np.random.default_rng(17).choice(dense.shape[0], 17000, replace=False))
    aside = synth.lidar_frame_at(yr.pose(-9.5, 1.8, 2), 8, beams=64, azimuths=1800)
    return np.ascontiguousarray(aside[::10][:700]), np.ascontiguousarray(dense[rows])


def d78l_lateral_drive():
    """-> poses: loop_yaw_ref.d78_drive() with the return leg a lane aside -- 30 frames out at y = 0.3, a turn over 18
    frames that also moves 1.5 m sideways, 30 frames back at y = 1.8 facing 183 degrees"""
    xs = [-20 + 0.6 * k for k in range(30)]
    return ([yr.pose(x, 0.3, 0) for x in xs]
            + [yr.pose(xs[-1], 0.3 + 1.5 * (k + 1) / 19, 183.0 * (k + 1) / 19) for k in range(18)]
            + [yr.pose(x, 1.8, 183.0) for x in reversed(xs)])


def l12_config():
    from lidar_slam_from_scratch_amd.loop_closure import LoopClosureConfig
    return LoopClosureConfig(yaw_guess=True, **L12_CONFIG)


def run_detector(detector, clouds, labels, add=None):
    """feed a drive to a detector -> every closure, in order.  add(detector, cloud, label): how a frame is added
    (default detector.add_frame(cloud, label))"""
    out = []
    for cloud, label in zip(clouds, labels):
        if add is None:
            detector.add_frame(cloud, label)
        else:
            add(detector, cloud, label)
        out += detector.detect()
    return out


if __name__ == "__main__":
    poses, labels = l12_lateral_drive()
    clouds = yr.scans(poses)
    for name, backend in (("ungated", yr.OracleBackend()), ("gate %.1f m" % L12_GATE, GatedOracleBackend(L12_GATE))):
        res = run_detector(yr.YawLoopClosureDetector(backend, l12_config()), clouds, labels)
        worst = 0.0
        from lidar_slam_from_scratch_amd import synth
        for c in res:
            dt, _ = synth.pose_delta(c.transform, yr.truth(poses, labels.index(c.query_frame), labels.index(c.match_frame)))
            worst = max(worst, dt)
        print("%-12s verifications %d, closures %d, queries closed %s, worst translation error %.3f m"
              % (name, len(backend.iterations), len(res), sorted({c.query_frame for c in res}), worst))
