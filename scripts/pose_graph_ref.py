#!/usr/bin/env python3
"""CPU restatement of the reference's pose-graph back end (core/pose_graph.cpp, GTSAM 4.x Levenberg-Marquardt), the
yardstick of the device optimiser (csrc/pose_graph.h).  numpy + scipy.sparse.linalg.splu.

Objective: 0.5 sum ||r||^2_Sigma over the factors, Pose3 with GTSAM_POSE3_EXPMAP / GTSAM_ROT3_EXPMAP (GTSAM's default
build), tangent order (omega, v):
    between  r = Log(Z^-1 X_i^-1 X_j)   dr/dxi_j = Jr^-1(r)   dr/dxi_i = -Jr^-1(r) Ad((X_i^-1 X_j)^-1)
    prior    r = Log(P^-1 X)            dr/dxi   = Jr^-1(r)
    retract  X (+) xi = X Exp(xi)
The LM policy lives in one place, `levenberg_marquardt`, each rule commented with the GTSAM function it restates.  The
device path (csrc/pose_graph.h, capi.hip icpmi_pose_graph_optimize) follows the same formulas and the same rules.

Poses are 4x4 arrays; batched helpers take (n, 3, 3) rotations and (n, 3) vectors."""
import math

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

SMALL_THETA = 0.1        # below: the series forms of the cancelling coefficients (same constant in csrc/se3.h)
TINY_THETA = 1e-8        # below: the series forms of sin(t)/t and (1 - cos t)/t^2

# stop reasons (icpmi_pose_graph_info.stop_reason, include/icp_mi355x.h)
STOP_NONE, STOP_ZERO_ERROR, STOP_MAX_ITERATIONS, STOP_RELATIVE, STOP_ABSOLUTE, STOP_LAMBDA_BOUND, \
    STOP_SMALL_COST_CHANGE, STOP_NOT_FINITE = range(8)


class PoseGraphConfig:
    """pose_graph.hpp:22-40"""

    def __init__(self, **kw):
        self.odom_rotation_sigma = 0.01
        self.odom_translation_sigma = 0.05
        self.prior_rotation_sigma = 0.001
        self.prior_translation_sigma = 0.001
        self.loop_rotation_sigma = 0.005
        self.loop_translation_sigma = 0.025
        self.max_iterations = 100
        self.relative_error_tol = 1e-5
        self.absolute_error_tol = 1e-5
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError(k)
            setattr(self, k, v)


# ---------------------------------------------------------------------------------------------------------- SE(3)

def hat(w):
    w = np.asarray(w, dtype=np.float64)
    z = np.zeros(w.shape[:-1])
    return np.stack([np.stack([z, -w[..., 2], w[..., 1]], -1),
                     np.stack([w[..., 2], z, -w[..., 0]], -1),
                     np.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def _theta(w):
    return np.sqrt(np.sum(w * w, axis=-1))


def _coefs(th):
    """A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3, D = 1/t^2 - (1 + cos t) / (2 t sin t)
    (the W^2 coefficient of V^-1 and of Jr^-1), E = (t^2 + 2 cos t - 2) / (2 t^4),
    F = (2 t - 3 sin t + t cos t) / (2 t^5) -- direct where stable, series below SMALL_THETA / TINY_THETA."""
    th = np.asarray(th, dtype=np.float64)
    t2 = th * th
    small, tiny = th < SMALL_THETA, th < TINY_THETA
    ts = np.where(tiny, 1.0, th)
    s, c = np.sin(ts), np.cos(ts)
    h = np.sin(0.5 * ts)
    A = np.where(tiny, 1.0 - t2 / 6.0, s / ts)
    B = np.where(tiny, 0.5 - t2 / 24.0, 2.0 * h * h / (ts * ts))
    tb = np.where(small, 1.0, th)
    sb, cb = np.sin(tb), np.cos(tb)
    hb = np.sin(0.5 * tb)
    C_s = 1.0 / 6 - t2 * (1.0 / 120 - t2 * (1.0 / 5040 - t2 * (1.0 / 362880 - t2 / 39916800)))
    D_s = 1.0 / 12 + t2 * (1.0 / 720 + t2 * (1.0 / 30240 + t2 * (1.0 / 1209600 + t2 / 47900160)))
    E_s = 1.0 / 24 - t2 * (1.0 / 720 - t2 * (1.0 / 40320 - t2 * (1.0 / 3628800 - t2 / 479001600)))
    F_s = 1.0 / 120 - t2 * (1.0 / 2520 - t2 * (1.0 / 120960 - t2 * (1.0 / 9979200 - t2 / 1245404160)))
    C = np.where(small, C_s, (tb - sb) / (tb * tb * tb))
    # 1/t^2 - s / (2 t (1 - c)), with 1 - c = 2 sin^2(t/2): stable up to t = pi
    D = np.where(small, D_s, 1.0 / (tb * tb) - sb / (4.0 * tb * hb * hb))
    E = np.where(small, E_s, (tb * tb + 2.0 * cb - 2.0) / (2.0 * ((tb * tb) * (tb * tb))))
    F = np.where(small, F_s, (2.0 * tb - 3.0 * sb + tb * cb) / (2.0 * (((tb * tb) * (tb * tb)) * tb)))
    return A, B, C, D, E, F


def so3_exp(w):
    w = np.asarray(w, dtype=np.float64)
    W = hat(w)
    A, B = _coefs(_theta(w))[:2]
    return np.eye(3) + A[..., None, None] * W + B[..., None, None] * (W @ W)


def so3_log(R):
    """Unit quaternion of R (Shepperd: the largest of w, x, y, z first), w >= 0, omega = 2 atan2(|q|, w) q / |q|.
    Accurate at every angle up to pi; R = I gives exactly 0."""
    R = np.asarray(R, dtype=np.float64)
    single = R.ndim == 2
    R = R.reshape(-1, 3, 3)
    out = np.empty((R.shape[0], 3))
    for k in range(R.shape[0]):
        out[k] = _so3_log1(R[k])
    return out[0] if single else out


def _so3_log1(R):
    r00, r01, r02 = R[0]
    r10, r11, r12 = R[1]
    r20, r21, r22 = R[2]
    tr = r00 + r11 + r22
    if tr >= r00 and tr >= r11 and tr >= r22:
        w = 0.5 * math.sqrt(1.0 + tr)
        f = 0.25 / w
        x, y, z = (r21 - r12) * f, (r02 - r20) * f, (r10 - r01) * f
    elif r00 >= r11 and r00 >= r22:
        x = 0.5 * math.sqrt(1.0 + r00 - r11 - r22)
        f = 0.25 / x
        w, y, z = (r21 - r12) * f, (r01 + r10) * f, (r02 + r20) * f
    elif r11 >= r22:
        y = 0.5 * math.sqrt(1.0 - r00 + r11 - r22)
        f = 0.25 / y
        w, x, z = (r02 - r20) * f, (r01 + r10) * f, (r12 + r21) * f
    else:
        z = 0.5 * math.sqrt(1.0 - r00 - r11 + r22)
        f = 0.25 / z
        w, x, y = (r10 - r01) * f, (r02 + r20) * f, (r12 + r21) * f
    if w < 0.0:
        w, x, y, z = -w, -x, -y, -z
    s = math.sqrt(x * x + y * y + z * z)
    if s < 1e-6 * w:
        q = s / w
        g = 2.0 / w * (1.0 - q * q / 3.0)
    else:
        g = 2.0 * math.atan2(s, w) / s
    return np.array([g * x, g * y, g * z])


def se3_exp(xi):
    """Pose3::Expmap: R = Exp(w), t = V(w) v."""
    xi = np.asarray(xi, dtype=np.float64)
    w, v = xi[..., :3], xi[..., 3:]
    W = hat(w)
    A, B, C = _coefs(_theta(w))[:3]
    W2 = W @ W
    R = np.eye(3) + A[..., None, None] * W + B[..., None, None] * W2
    V = np.eye(3) + B[..., None, None] * W + C[..., None, None] * W2
    T = np.zeros(xi.shape[:-1] + (4, 4))
    T[..., :3, :3] = R
    T[..., :3, 3] = np.einsum("...ij,...j->...i", V, v)
    T[..., 3, 3] = 1.0
    return T


def se3_log(T):
    """Pose3::Logmap: w = Log(R), v = V(w)^-1 t with V^-1 = I - W/2 + D W^2."""
    T = np.asarray(T, dtype=np.float64)
    w = so3_log(T[..., :3, :3])
    W = hat(w)
    D = _coefs(_theta(w))[3]
    Vinv = np.eye(3) - 0.5 * W + D[..., None, None] * (W @ W)
    return np.concatenate([w, np.einsum("...ij,...j->...i", Vinv, T[..., :3, 3])], -1)


def se3_jr_inv(xi):
    """Pose3::LogmapDerivative: the inverse right Jacobian [Jw^-1, 0; -Jw^-1 Q Jw^-1, Jw^-1] with
    Jw^-1 = I + W/2 + D W^2 and Q the right-Jacobian coupling block (Pose3::ComputeQforExpmapDerivative):
    Q = -V/2 + C (WV + VW - WVW) - E (WWV + VWW - 3 WVW) + F (WVWW + WWVW)."""
    xi = np.asarray(xi, dtype=np.float64)
    w, v = xi[..., :3], xi[..., 3:]
    W, V = hat(w), hat(v)
    _, _, C, D, E, F = _coefs(_theta(w))
    e = lambda a: a[..., None, None]  # noqa: E731
    Jwi = np.eye(3) + 0.5 * W + e(D) * (W @ W)
    WV, VW, WW = W @ V, V @ W, W @ W
    WVW = WV @ W
    Q = -0.5 * V + e(C) * (WV + VW - WVW) - e(E) * (WW @ V + VW @ W - 3.0 * WVW) + e(F) * (WVW @ W + WW @ VW)
    J = np.zeros(xi.shape[:-1] + (6, 6))
    J[..., :3, :3] = Jwi
    J[..., 3:, 3:] = Jwi
    J[..., 3:, :3] = -(Jwi @ Q @ Jwi)
    return J


def adjoint(T):
    """Pose3::AdjointMap in (w, v) order: [R, 0; t^ R, R]."""
    T = np.asarray(T, dtype=np.float64)
    R, t = T[..., :3, :3], T[..., :3, 3]
    Ad = np.zeros(T.shape[:-2] + (6, 6))
    Ad[..., :3, :3] = R
    Ad[..., 3:, 3:] = R
    Ad[..., 3:, :3] = hat(t) @ R
    return Ad


def inverse(T):
    T = np.asarray(T, dtype=np.float64)
    out = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -np.einsum("...ij,...j->...i", Rt, T[..., :3, 3])
    out[..., 3, 3] = 1.0
    return out


# ------------------------------------------------------------------------------------------------------- factors

def factor_residuals(kind, fi, fj, Z, X):
    """Unwhitened residuals and Jacobians of every factor at values X (n, 4, 4); kind 0 prior, 1 between.
    Returns r (F, 6), Ji (F, 6, 6), Jj (F, 6, 6) (Jj zero for priors)."""
    Xi = X[fi]
    F = len(kind)
    between = kind == 1
    rel = Xi.copy()                                      # prior: P^-1 X;  between: Z^-1 (X_i^-1 X_j)
    if between.any():
        rel[between] = inverse(Xi[between]) @ X[fj[between]]
    E = inverse(Z) @ rel
    r = se3_log(E)
    Jr = se3_jr_inv(r)
    Ji = Jr.copy()
    Jj = np.zeros((F, 6, 6))
    if between.any():
        Jj[between] = Jr[between]
        Ji[between] = -(Jr[between] @ adjoint(inverse(rel[between])))
    return r, Ji, Jj


def factor_errors(kind, fi, fj, Z, inv_sigma, X):
    r = factor_residuals(kind, fi, fj, Z, X)[0] * inv_sigma
    return 0.5 * np.sum(r * r, axis=1)


def total_error(kind, fi, fj, Z, inv_sigma, X):
    return float(np.sum(factor_errors(kind, fi, fj, Z, inv_sigma, X)))


def retract(X, delta):
    return X @ se3_exp(delta.reshape(-1, 6))


# ----------------------------------------------------------------------------------------------------- LM policy

EPS = np.finfo(np.float64).eps


def _solve(H, g, lam, ordering):
    """(H + lam I) delta = -g by sparse LU without row pivoting (diag_pivot_thresh 0, symmetric mode): on an SPD
    matrix its pivots are those of the Cholesky; a non-positive or non-finite one is an unsolved system, as GTSAM's
    IndeterminantLinearSystemException (caught in LevenbergMarquardtOptimizer::tryLambda).  ordering "DENSE": the same
    matrix by numpy's dense Cholesky, a third rounding of the same step for the tests' spread."""
    n = H.shape[0]
    M = (H + lam * sp.identity(n, format="csc")).tocsc()
    if ordering == "DENSE":
        try:
            L = np.linalg.cholesky(M.toarray())
        except np.linalg.LinAlgError:
            return None
        d = sla.solve_triangular(L, sla.solve_triangular(L, -g, lower=True), lower=True, trans="T")
        return d if np.all(np.isfinite(d)) else None
    try:
        lu = spla.splu(M, permc_spec=ordering, diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    except RuntimeError:
        return None
    piv = lu.U.diagonal()
    if not np.all(np.isfinite(piv)) or np.any(piv <= 0.0):
        return None
    d = lu.solve(-g)
    return d if np.all(np.isfinite(d)) else None


def _linearize(kind, fi, fj, Z, inv_sigma, X):
    """Whitened residual b = -r/sigma and Jacobians A = J/sigma (noiseModel::Diagonal::WhitenSystem); H = A^T A,
    g = A^T r/sigma summed per block (HessianFactor of a JacobianFactor)."""
    r, Ji, Jj = factor_residuals(kind, fi, fj, Z, X)
    rw = r * inv_sigma
    Ai = Ji * inv_sigma[:, :, None]
    Aj = Jj * inv_sigma[:, :, None]
    return rw, Ai, Aj


def _normal_equations(n, kind, fi, fj, rw, Ai, Aj):
    rows, cols, vals = [], [], []
    g = np.zeros((n, 6))
    bi = np.arange(6)

    def add(blocks, a, b):
        rr = (6 * a[:, None, None] + bi[None, :, None]) * np.ones((1, 1, 6), dtype=np.int64)
        cc = (6 * b[:, None, None] + bi[None, None, :]) * np.ones((1, 6, 1), dtype=np.int64)
        rows.append(rr.ravel())
        cols.append(cc.ravel())
        vals.append(blocks.ravel())

    AiT = np.swapaxes(Ai, 1, 2)
    add(AiT @ Ai, fi, fi)
    np.add.at(g, fi, np.einsum("fij,fj->fi", AiT, rw))
    bt = kind == 1
    if bt.any():
        AjT = np.swapaxes(Aj[bt], 1, 2)
        Hij = AiT[bt] @ Aj[bt]
        add(AjT @ Aj[bt], fj[bt], fj[bt])
        add(Hij, fi[bt], fj[bt])
        add(np.swapaxes(Hij, 1, 2), fj[bt], fi[bt])
        np.add.at(g, fj[bt], np.einsum("fij,fj->fi", AjT, rw[bt]))
    H = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * n, 6 * n))
    return H.tocsc(), g.ravel()


def _linear_error(kind, fi, fj, rw, Ai, Aj, delta):
    """GaussianFactorGraph::error(delta) = 0.5 sum ||A delta - b||^2 with b = -rw."""
    d = delta.reshape(-1, 6)
    e = np.einsum("fij,fj->fi", Ai, d[fi]) + rw
    bt = kind == 1
    e[bt] += np.einsum("fij,fj->fi", Aj[bt], d[fj[bt]])
    return float(np.sum(0.5 * np.sum(e * e, axis=1)))


class LMStats:
    def __init__(self):
        self.iterations = 0
        self.inner_trials = 0
        self.initial_error = 0.0
        self.final_error = 0.0
        self.final_lambda = 0.0
        self.stop_reason = STOP_NONE
        self.history = []
        self.min_margin = math.inf   # smallest relative distance of any stopping / acceptance test from its threshold


def _margin(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def levenberg_marquardt(kind, fi, fj, Z, inv_sigma, X0, cfg, ordering="COLAMD", linearize=None, errors=None):
    """LevenbergMarquardtOptimizer::optimize() with LevenbergMarquardtParams' defaults and the caller's
    max_iterations / relativeErrorTol / absoluteErrorTol (pose_graph.cpp:153-157).  Returns (X, LMStats).
    `linearize` and `errors` replace `_linearize` and `factor_errors` (same arguments, same returns): a robust noise
    model whitens the system and prices a factor differently (scripts/pose_graph_loss_ref.py); the policy is this one."""
    linearize = linearize or _linearize
    errors = errors or factor_errors
    lam, lam_factor, lam_lower, lam_upper = 1e-5, 10.0, 0.0, 1e5   # LevenbergMarquardtParams: lambdaInitial,
    min_fidelity = 1e-3                                             # lambdaFactor, lambdaLowerBound, lambdaUpperBound,
    rel_tol, abs_tol, err_tol = cfg.relative_error_tol, cfg.absolute_error_tol, 0.0   # minModelFidelity; errorTol 0
    n = X0.shape[0]
    X = X0.copy()
    st = LMStats()
    error = float(np.sum(errors(kind, fi, fj, Z, inv_sigma, X)))
    st.initial_error = error
    st.history.append(error)
    # NonlinearOptimizer::defaultOptimize: nothing to do when the error is already <= errorTol or no iteration is allowed
    if error <= err_tol:
        st.stop_reason = STOP_ZERO_ERROR
    elif st.iterations >= cfg.max_iterations:
        st.stop_reason = STOP_MAX_ITERATIONS
    while st.stop_reason == STOP_NONE:
        current = error
        # LevenbergMarquardtOptimizer::iterate: linearise once, then tryLambda until it returns true
        rw, Ai, Aj = linearize(kind, fi, fj, Z, inv_sigma, X)
        H, g = _normal_equations(n, kind, fi, fj, rw, Ai, Aj)
        old_lin = _linear_error(kind, fi, fj, rw, Ai, Aj, np.zeros(6 * n))   # linear.error(VectorValues::Zero)
        stepped, inner_stop = False, STOP_NONE
        while True:
            st.inner_trials += 1
            # tryLambda: buildDampedSystem adds lambda I (diagonalDamping off), then solve
            delta = _solve(H, g, lam, ordering)
            step_ok, stop_search = False, False
            if delta is not None:
                new_lin = _linear_error(kind, fi, fj, rw, Ai, Aj, delta)
                lin_change = old_lin - new_lin
                if lin_change >= 0.0:                                           # tryLambda: the step is valid
                    Xn = retract(X, delta)
                    new_err = float(np.sum(errors(kind, fi, fj, Z, inv_sigma, Xn)))
                    cost_change = current - new_err
                    if lin_change > EPS * old_lin:
                        fidelity = cost_change / lin_change                     # tryLambda: modelFidelity
                        step_ok = fidelity > min_fidelity
                        st.min_margin = min(st.min_margin, _margin(fidelity, min_fidelity))
                    else:
                        step_ok = True                                          # linearised change ~ 0
                    # tryLambda: stop searching lambda once |costChange| < relativeErrorTol * error
                    stop_search = abs(cost_change) < rel_tol * current
                    st.min_margin = min(st.min_margin, _margin(abs(cost_change), rel_tol * current))
            if step_ok:
                # State::decreaseLambda (useFixedLambdaFactor): lambda /= lambdaFactor, bounded below
                lam = max(lam_lower, lam / lam_factor)
                X, error = Xn, new_err
                st.iterations += 1
                stepped = True
                break
            if stop_search:
                inner_stop = STOP_SMALL_COST_CHANGE                             # tryLambda returns true
                break
            lam *= lam_factor                                                   # State::increaseLambda
            if lam >= lam_upper:                                                # tryLambda: lambda too big, give up
                inner_stop = STOP_LAMBDA_BOUND
                break
        st.history.append(error)
        # defaultOptimize's loop condition: iterations < maxIterations && !checkConvergence(...) && isfinite(error)
        if not stepped:
            st.stop_reason = inner_stop          # the error did not move: checkConvergence holds (absolute decrease 0)
        elif st.iterations >= cfg.max_iterations:
            st.stop_reason = STOP_MAX_ITERATIONS
        elif not math.isfinite(current):
            st.stop_reason = STOP_NOT_FINITE
        else:
            # checkConvergence (NonlinearOptimizer.cpp)
            abs_dec = current - error
            rel_dec = abs_dec / current
            st.min_margin = min(st.min_margin, _margin(rel_dec, rel_tol), _margin(abs_dec, abs_tol))
            if error <= err_tol:
                st.stop_reason = STOP_ZERO_ERROR
            elif rel_tol and rel_dec <= rel_tol:
                st.stop_reason = STOP_RELATIVE
            elif abs_dec <= abs_tol:
                st.stop_reason = STOP_ABSOLUTE
    st.final_error = error
    st.final_lambda = lam
    return X, st


# ----------------------------------------------------------------------------------------------------- PoseGraph

class PoseGraphError(ValueError):
    """The cases the C ABI reports as ICPMI_ERR_ARG."""


def _check_T(T):
    T = np.asarray(T, dtype=np.float64)
    if T.shape != (4, 4) or not np.all(np.isfinite(T)):
        raise PoseGraphError("transform must be a finite 4x4")
    return T.copy()


class PoseGraph:
    """slam::PoseGraph (pose_graph.hpp:49-147, pose_graph.cpp) on the restatement above."""

    def __init__(self, config=None):
        self.config = config or PoseGraphConfig()
        self.factors = []            # (kind, i, j, Z, sigmas)
        self.initial = {}            # index -> 4x4
        self.optimized_values = {}
        self.num_poses = 0
        self.num_loop_closures = 0
        self.optimized = False
        self.final_error = 0.0
        self.iterations = 0
        self.stats = None

    def add_prior(self, index, pose):
        """pose_graph.cpp:58-79 (does not clear optimized_)"""
        pose = _check_T(pose)
        c = self.config
        s = [c.prior_rotation_sigma] * 3 + [c.prior_translation_sigma] * 3
        self.factors.append((0, int(index), -1, pose, np.array(s)))
        if index not in self.initial:
            self.initial[int(index)] = pose
            self.num_poses = max(self.num_poses, int(index) + 1)

    def add_odometry_factor(self, i, j, Z, fitness=0.0):
        """pose_graph.cpp:81-116: sigma scaled by 1 + 10 fitness; j gets X_i Z if it has no estimate"""
        Z = _check_T(Z)
        if i == j or not math.isfinite(fitness):
            raise PoseGraphError("bad factor")
        if j not in self.initial and i not in self.initial:
            raise PoseGraphError("pose %d has no estimate" % i)     # Values::at throws (pose_graph.cpp:104)
        c = self.config
        scale = 1.0 + fitness * 10.0
        s = [c.odom_rotation_sigma * scale] * 3 + [c.odom_translation_sigma * scale] * 3
        self.factors.append((1, int(i), int(j), Z, np.array(s)))
        if j not in self.initial:
            Xi = self.initial[i]
            Xj = np.eye(4)
            Xj[:3, :3] = Xi[:3, :3] @ Z[:3, :3]                     # Pose3::compose
            Xj[:3, 3] = Xi[:3, :3] @ Z[:3, 3] + Xi[:3, 3]
            self.initial[int(j)] = Xj
            self.num_poses = max(self.num_poses, int(j) + 1)
        self.optimized = False

    def add_loop_closure(self, i, j, Z):
        """pose_graph.cpp:118-141: no estimate added"""
        Z = _check_T(Z)
        if i == j:
            raise PoseGraphError("bad factor")
        c = self.config
        s = [c.loop_rotation_sigma] * 3 + [c.loop_translation_sigma] * 3
        self.factors.append((1, int(i), int(j), Z, np.array(s)))
        self.num_loop_closures += 1
        self.optimized = False

    def arrays(self):
        """(keys, kind, fi, fj, Z, inv_sigma, X0) in compact order, or None when a factor names a missing estimate."""
        keys = sorted(self.initial)
        pos = {k: p for p, k in enumerate(keys)}
        try:
            fi = np.array([pos[f[1]] for f in self.factors], dtype=np.int64)
            fj = np.array([pos[f[2]] if f[0] == 1 else 0 for f in self.factors], dtype=np.int64)
        except KeyError:
            return None
        kind = np.array([f[0] for f in self.factors], dtype=np.int64)
        Z = np.stack([f[3] for f in self.factors])
        inv_sigma = 1.0 / np.stack([f[4] for f in self.factors])
        X0 = np.stack([self.initial[k] for k in keys])
        return keys, kind, fi, fj, Z, inv_sigma, X0

    def optimize(self, ordering="COLAMD"):
        """pose_graph.cpp:147-171: always from the initial estimates"""
        if self.num_poses == 0:
            return False
        a = self.arrays()
        if a is None:
            return False                           # the reference's catch: a factor on a pose with no estimate
        keys, kind, fi, fj, Z, inv_sigma, X0 = a
        X, st = levenberg_marquardt(kind, fi, fj, Z, inv_sigma, X0, self.config, ordering)
        self.optimized_values = {k: X[p] for p, k in enumerate(keys)}
        self.final_error, self.iterations, self.stats = st.final_error, st.iterations, st
        self.optimized = True
        return True

    def _values(self):
        return self.optimized_values if self.optimized else self.initial

    def get_pose(self, index):
        """pose_graph.cpp:177-186"""
        v = self._values()
        if index not in v:
            raise PoseGraphError("Pose index %d not found" % index)
        return v[index].copy()

    def get_all_poses(self):
        """pose_graph.cpp:188-200: 0..num_poses-1, gaps skipped"""
        v = self._values()
        return [v[i].copy() for i in range(self.num_poses) if i in v]

    def size(self):
        return self.num_poses

    def loop_closure_count(self):
        return self.num_loop_closures
