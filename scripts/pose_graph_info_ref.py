#!/usr/bin/env python3
"""CPU restatement of the pose graph's full-information between factors (csrc/pose_graph_info.h): GTSAM's
noiseModel::Gaussian::Information, which keeps the upper Cholesky factor R of the information L = R^T R and whitens
with it, rw = R r, A = R J.  The LM policy is pose_graph_ref's, untouched, through its two hooks; the loop loss is
pose_graph_loss_ref's, on d = ||R r||.

Frames.  ICP's step is a left perturbation of its result T in the target frame, p' = p + r x p + t with x = [r; t], and
JtJ = sum J^T J, J = [(p x n)^T, n^T], is the curvature of its cost in x.  The graph's between factor is
Log(Z^-1 X_i^-1 X_j) with a right perturbation in (omega, v) order, entered with Z = T, i = the target's pose, j = the
source's.  To first order Exp(x) T = T Exp(Ad_{T^-1} x), so a right step xi moves the cost as x = Ad_T xi does:
    L = Ad_T^T (JtJ / sigma^2) Ad_T + diag(1 / floor_r^2 x 3, 1 / floor_t^2 x 3),   Ad_T = [[R, 0], [t^ R, R]].
For an edge entered the other way round, Z = T^-1 from the source's pose, the same JtJ is right-frame information as it
stands: T^-1 Exp(-x) is a right perturbation of T^-1 and the quadratic form does not see the sign.

`information_from_icp` and `cholesky_upper` repeat csrc/pose_graph_info_host.h operation for operation on Python
floats (IEEE doubles, no FMA): their results are bit-equal to the library's.

Run as a program: the table of DESIGN 7.13 (a ring with anisotropic odometry noise, isotropic sigmas against the true
information on the edges)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_loss_ref as L  # noqa: E402
import pose_graph_ref as R  # noqa: E402

SYM_TOL = 1e-9       # kPgInfoSymTol (csrc/pose_graph_info_host.h, where it is derived)


def adjoint_of(T):
    """Ad_T in (omega, v) order: x = Ad_T xi maps the graph's right perturbation to ICP's left one."""
    return R.adjoint(np.asarray(T, dtype=np.float64))


def information_from_icp(JtJ, T, sigma, floor_rotation_sigma=0.0, floor_translation_sigma=0.0):
    """icpmi_information_from_icp, in its operation order.  Raises PoseGraphError where it returns ICPMI_ERR_ARG."""
    JtJ = np.asarray(JtJ, dtype=np.float64).reshape(6, 6)
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    fr, ft = float(floor_rotation_sigma), float(floor_translation_sigma)
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0.0):
        raise R.PoseGraphError("sigma must be finite and > 0")
    if not (math.isfinite(fr) and math.isfinite(ft) and fr >= 0.0 and ft >= 0.0):
        raise R.PoseGraphError("a floor is 0 or finite and > 0")
    if not (np.all(np.isfinite(JtJ)) and np.all(np.isfinite(T))):
        raise R.PoseGraphError("non-finite JtJ or T")
    J = [[float(JtJ[a, b]) for b in range(6)] for a in range(6)]
    Tm = [[float(T[a, b]) for b in range(4)] for a in range(4)]
    t = [Tm[0][3], Tm[1][3], Tm[2][3]]
    hat = [[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]]
    Ad = [[0.0] * 6 for _ in range(6)]
    for i in range(3):
        for j in range(3):
            r = Tm[i][j]
            Ad[i][j] = r
            Ad[3 + i][3 + j] = r
            Ad[3 + i][j] = (hat[i][0] * Tm[0][j] + hat[i][1] * Tm[1][j]) + hat[i][2] * Tm[2][j]
    s2 = sigma * sigma
    M = [[(J[a][b] if a <= b else J[b][a]) / s2 for b in range(6)] for a in range(6)]
    P = [[0.0] * 6 for _ in range(6)]
    for a in range(6):
        for b in range(6):
            s = 0.0
            for l in range(6):
                s = s + M[a][l] * Ad[l][b]
            P[a][b] = s
    out = np.zeros((6, 6))
    for a in range(6):
        for b in range(a, 6):
            s = 0.0
            for l in range(6):
                s = s + Ad[l][a] * P[l][b]
            out[a, b] = s
            out[b, a] = s
    for a in range(3):
        if fr > 0.0:
            out[a, a] = out[a, a] + 1.0 / (fr * fr)
        if ft > 0.0:
            out[3 + a, 3 + a] = out[3 + a, 3 + a] + 1.0 / (ft * ft)
    return out


def cholesky_upper(info):
    """pg_info_cholesky: the checks of icpmi_pose_graph_add_*_information, then R (6 x 6 upper) with info = R^T R.
    Raises PoseGraphError where they return ICPMI_ERR_ARG."""
    A = np.asarray(info, dtype=np.float64)
    if A.shape != (6, 6) or not np.all(np.isfinite(A)):
        raise R.PoseGraphError("information must be a finite 6x6")
    if not np.all(np.diag(A) > 0.0):
        raise R.PoseGraphError("information is not positive definite")
    for a in range(6):
        for b in range(a + 1, 6):
            if not abs(A[a, b] - A[b, a]) <= SYM_TOL * math.sqrt(A[a, a] * A[b, b]):
                raise R.PoseGraphError("information is not symmetric")
    U = np.zeros((6, 6))
    for a in range(6):
        d = float(A[a, a])
        for k in range(a):
            d = d - U[k, a] * U[k, a]
        if not (d > 0.0 and math.isfinite(d)):
            raise R.PoseGraphError("information is not positive definite")
        p = math.sqrt(d)
        U[a, a] = p
        for b in range(a + 1, 6):
            s = float(A[a, b])
            for k in range(a):
                s = s - U[k, a] * U[k, b]
            U[a, b] = s / p
    return U


def _whiten(rw_or_J, inv_sigma, slot, Rs):
    """Rows whitened: a diagonal factor by its inv_sigma, an information factor (slot >= 0) by R of that slot."""
    x = np.asarray(rw_or_J)
    vec = x.ndim == 2
    out = x * (inv_sigma if vec else inv_sigma[:, :, None])
    m = slot >= 0
    if m.any():
        Rm = Rs[slot[m]]
        out[m] = np.einsum("fab,fb->fa", Rm, x[m]) if vec else Rm @ x[m]
    return out


def info_linearize(slot, Rs, is_loop=None, kind=L.LOSS_NONE, k=0.0, watch=None):
    """The `linearize` hook: Gaussian::WhitenSystem per factor, then Robust's sqrt(w) on the loop factors' rows."""
    def linearize(fkind, fi, fj, Z, inv_sigma, X):
        r, Ji, Jj = R.factor_residuals(fkind, fi, fj, Z, X)
        rw, Ai, Aj = _whiten(r, inv_sigma, slot, Rs), _whiten(Ji, inv_sigma, slot, Rs), _whiten(Jj, inv_sigma, slot, Rs)
        if is_loop is not None and kind != L.LOSS_NONE:
            d = L._distance(rw[is_loop])
            if watch is not None:
                watch.see(d, kind, k)
            sw = L.loss_weight_rho(d, kind, k)[2]
            rw[is_loop] = rw[is_loop] * sw[:, None]
            Ai[is_loop] = Ai[is_loop] * sw[:, None, None]
            Aj[is_loop] = Aj[is_loop] * sw[:, None, None]
        return rw, Ai, Aj
    return linearize


def info_factor_errors(slot, Rs, is_loop=None, kind=L.LOSS_NONE, k=0.0, watch=None):
    """The `errors` hook: 0.5 ||R r||^2, and rho(||R r||) for a loop factor under a loss."""
    def errors(fkind, fi, fj, Z, inv_sigma, X):
        rw = _whiten(R.factor_residuals(fkind, fi, fj, Z, X)[0], inv_sigma, slot, Rs)
        e = 0.5 * np.sum(rw * rw, axis=1)
        if is_loop is not None and kind != L.LOSS_NONE:
            d = L._distance(rw[is_loop])
            if watch is not None:
                watch.see(d, kind, k)
            e[is_loop] = L.loss_weight_rho(d, kind, k)[1]
        return e
    return errors


class PoseGraph(L.PoseGraph):
    """pose_graph_loss_ref.PoseGraph with icpmi_pose_graph_add_odometry_information / _add_loop_closure_information."""

    def __init__(self, config=None):
        super().__init__(config)
        self.info_R = {}             # position in self.factors -> R (6 x 6 upper)

    def add_odometry_information(self, i, j, Z, info):
        U = cholesky_upper(info)     # refused before anything changes
        self.add_odometry_factor(i, j, Z, 0.0)
        self.info_R[len(self.factors) - 1] = U

    def add_loop_closure_information(self, i, j, Z, info):
        U = cholesky_upper(info)
        self.add_loop_closure(i, j, Z)
        self.info_R[len(self.factors) - 1] = U

    def _slots(self):
        slot = np.full(len(self.factors), -1, dtype=np.int64)
        order = sorted(self.info_R)
        slot[order] = np.arange(len(order))
        Rs = np.stack([self.info_R[p] for p in order]) if order else np.zeros((0, 6, 6))
        return slot, Rs

    def optimize(self, ordering="COLAMD"):
        if not self.info_R:
            return super().optimize(ordering)
        if self.num_poses == 0:
            return False
        a = self.arrays()
        if a is None:
            return False
        keys, kind, fi, fj, Z, inv_sigma, X0 = a
        slot, Rs = self._slots()
        watch = L.HuberWatch()
        loss = (self._is_loop(), self.loss_kind, self.loss_scale, watch) if self.loop_factors else ()
        X, st = R.levenberg_marquardt(kind, fi, fj, Z, inv_sigma, X0, self.config, ordering,
                                      linearize=info_linearize(slot, Rs, *loss),
                                      errors=info_factor_errors(slot, Rs, *loss))
        st.min_margin = min(st.min_margin, watch.min_margin)
        self.optimized_values = {k: X[p] for p, k in enumerate(keys)}
        self.final_error, self.iterations, self.stats = st.final_error, st.iterations, st
        self.optimized = True
        return True

    def loop_distances_at(self, poses):
        keys, kind, fi, fj, Z, inv_sigma, _ = self.arrays()
        X = np.stack([poses[k] for k in keys])
        lf = np.array(self.loop_factors, dtype=np.int64)
        if not len(lf):
            return np.zeros(0)
        slot, Rs = self._slots()
        r = R.factor_residuals(kind[lf], fi[lf], fj[lf], Z[lf], X)[0]
        return L._distance(_whiten(r, inv_sigma[lf], slot[lf], Rs))


def apply(g, ops):
    """pose_graph_loss_ref.apply plus ("odom_info", i, j, Z, info) and ("loop_info", i, j, Z, info)."""
    for op in ops:
        if op[0] == "odom_info":
            g.add_odometry_information(op[1], op[2], op[3], op[4])
        elif op[0] == "loop_info":
            g.add_loop_closure_information(op[1], op[2], op[3], op[4])
        else:
            L.apply(g, [op])


# ------------------------------------------------------------------------------------------- the table of DESIGN 7.13
# A ring driven once round, closed by a few accurate closures.  Every odometry edge is anisotropic as a registration in a
# street leaves it -- looser along the direction of travel (the body x axis) than across it, tight in rotation -- and one
# stretch of twenty edges is a corridor, where along-track is all but unobserved.  One graph weighs every edge by the
# config's isotropic sigmas, the other by the inverse of the covariance each edge's noise was drawn from: it knows where
# the closing error belongs.

RING_N, RING_RADIUS = 200, 40.0
RING_ROT, RING_CROSS, RING_ALONG, RING_ALONG_CORRIDOR = 2e-4, 0.003, 0.02, 0.4     # rad, m, m, m
RING_CORRIDOR = range(80, 100)                                                      # edges (k, k + 1)
RING_LOOPS = [(0, 199), (2, 197), (5, 195), (10, 190)]
RING_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)


def _ring_pose(k, n=RING_N, radius=RING_RADIUS):
    a = 2.0 * math.pi * k / n
    T = np.eye(4)
    c, s = math.cos(a + 0.5 * math.pi), math.sin(a + 0.5 * math.pi)     # x along the tangent: the direction of travel
    T[:3, :3] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = [radius * math.cos(a), radius * math.sin(a), 0.0]
    return T


def ring_edge_sigmas(k):
    """(omega, v) sigmas of odometry edge (k, k + 1)"""
    along = RING_ALONG_CORRIDOR if k in RING_CORRIDOR else RING_ALONG
    return np.array([RING_ROT] * 3 + [along, RING_CROSS, RING_CROSS])


def anisotropic_ring(seed, information):
    """-> (ops, ground truth).  information False: ("odom", ..) / ("loop", ..) under the config's sigmas; True: the same
    measurements as ("odom_info", ..) / ("loop_info", ..) with the inverse covariance they were drawn from."""
    rng = np.random.default_rng(seed)
    gt = [_ring_pose(k) for k in range(RING_N)]
    loop_s = np.array([0.001] * 3 + [0.01] * 3)
    Ll = np.diag(1.0 / loop_s ** 2)
    ops = [("prior", 0, gt[0])]
    for k in range(RING_N - 1):
        sig = ring_edge_sigmas(k)
        Z = np.linalg.inv(gt[k]) @ gt[k + 1] @ R.se3_exp(rng.normal(0.0, 1.0, 6) * sig)
        ops.append(("odom_info", k, k + 1, Z, np.diag(1.0 / sig ** 2)) if information else ("odom", k, k + 1, Z, 0.0))
    for i, j in RING_LOOPS:
        Z = np.linalg.inv(gt[i]) @ gt[j] @ R.se3_exp(rng.normal(0.0, 1.0, 6) * loop_s)
        ops.append(("loop_info", i, j, Z, Ll) if information else ("loop", i, j, Z))
    return ops, gt


def ate(poses, gt):
    """RMS translation error against ground truth (both start from the same prior: no alignment)."""
    d = np.stack(poses)[:, :3, 3] - np.stack(gt)[:, :3, 3]
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1))))


def ring_ates(seed):
    out = []
    for information in (False, True):
        ops, gt = anisotropic_ring(seed, information)
        g = PoseGraph()
        apply(g, ops)
        assert g.optimize()
        out.append(ate(g.get_all_poses(), gt))
    return tuple(out)


def main():
    print("| seed | ATE, isotropic sigmas [m] | ATE, information edges [m] |")
    print("|---|---|---|")
    for seed in RING_SEEDS:
        iso, info = ring_ates(seed)
        print("| %d | %.4f | %.4f |" % (seed, iso, info))


if __name__ == "__main__":
    main()
