"""The CPU restatement of the pose graph's information edges (scripts/pose_graph_info_ref.py): the frame in which a
registration's normal matrix becomes an edge's information, the whitening, the diagonal special case against
scripts/pose_graph_ref.py, and what the feature is for -- a ring whose closing error belongs to a corridor.  Runs on
the CPU.

The frame test.  2,000 source points p_i in a room corner (three orthogonal planes, |p_i| <= RHO_S), their targets
q_i = T p_i + (noise along the plane's normal n_i), correspondences and normals fixed.  b_i(X) = (q_i - X p_i) . n_i.
For a right perturbation X = T Exp(xi), T Exp(xi) p = T p + R (w x p + v) + R d2 with
    |d2| <= 1/2 |w|^2 |p| + 1/2 |w| |v| + 1/6 |w|^2 |v| <= |xi|^2 (RHO_S / 2 + 1/4 + |xi| / 6) =: E2
(Exp's coefficients: (1 - cos t) / t^2 <= 1/2, (t - sin t) / t^3 <= 1/6, and |w| |v| <= |xi|^2 / 2), and the first-order
part is exactly ICP's left step x = Ad_T xi applied to the moved point T p.  So b_i(xi) = b_i - J_i x - e_i with
|e_i| <= E2, and
    | sum b_i(xi)^2 - (sum b^2 - 2 x^T J^T b + x^T J^T J x) | = | sum (2 e_i (b_i - J_i x) + e_i^2) |
                                                             <= n (2 E2 (max|b| + JMAX |x|) + E2^2)
with JMAX = sqrt(RHO_T^2 + 1) >= |J_i| (RHO_T bounds the moved points) and |x| the mapped step's norm.  The residuals are
drawn at 1e-4 m, the size of |xi|, so every term of the bound is third order in |xi|: ~1e-8 here, where a wrong map of xi
(Ad of the inverse, or the transpose) moves x^T J^T J x by second order."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import pose_graph_info_ref as I  # noqa: E402
import pose_graph_ref as R  # noqa: E402
from test_gpu_pose_graph import chain_ops, ring_ops  # noqa: E402

N_POINTS, XI_NORM, B_NOISE = 2000, 1e-4, 1e-4


def corner_pair(seed=0):
    """-> (p, q, n, T): source points, their fixed targets and normals, and the pose the registration ended at."""
    rng = np.random.default_rng(seed)
    T = R.se3_exp(np.array([0.3, -0.5, 0.8, 2.0, -1.5, 0.7]))
    moved = np.zeros((N_POINTS, 3))          # points on the planes x = 0, y = 0, z = 0 of the target frame, 0..5 m
    nrm = np.zeros((N_POINTS, 3))
    for i in range(N_POINTS):
        a = i % 3
        moved[i] = rng.uniform(0.0, 5.0, 3)
        moved[i, a] = 0.0
        nrm[i, a] = 1.0
    q = moved + nrm * rng.normal(0.0, B_NOISE, (N_POINTS, 1))
    Ti = R.inverse(T)
    p = moved @ Ti[:3, :3].T + Ti[:3, 3]
    return p, q, nrm, T


def residuals(X, p, q, nrm):
    return np.sum((q - (p @ X[:3, :3].T + X[:3, 3])) * nrm, axis=1)


def normal_equations(T, p, q, nrm):
    m = p @ T[:3, :3].T + T[:3, 3]
    J = np.concatenate([np.cross(m, nrm), nrm], axis=1)
    b = np.sum((q - m) * nrm, axis=1)
    return J.T @ J, J.T @ b, float(b @ b), m, b


def third_order_bound(rho_s, rho_t, bmax, xnorm):
    e2 = XI_NORM ** 2 * (0.5 * rho_s + 0.25 + XI_NORM / 6.0)
    return N_POINTS * (2.0 * e2 * (bmax + math.sqrt(rho_t ** 2 + 1.0) * xnorm) + e2 * e2) + 1e-12


def _xis(count=20, seed=5):
    rng = np.random.default_rng(seed)
    xi = rng.normal(0.0, 1.0, (count, 6))
    return xi * (XI_NORM / np.linalg.norm(xi, axis=1))[:, None]


def test_frame_of_the_information():
    p, q, nrm, T = corner_pair()
    JtJ, Jtb, bb, moved, b = normal_equations(T, p, q, nrm)
    rho_s, rho_t, bmax = np.linalg.norm(p, axis=1).max(), np.linalg.norm(moved, axis=1).max(), np.abs(b).max()
    Ad, Adi = I.adjoint_of(T), I.adjoint_of(R.inverse(T))
    worst, miss_inv, miss_tr = 0.0, [], []
    for xi in _xis():
        exact = float(np.sum(residuals(T @ R.se3_exp(xi), p, q, nrm) ** 2))

        def model(x):
            return bb - 2.0 * float(x @ Jtb) + float(x @ JtJ @ x)

        x = Ad @ xi
        bound = third_order_bound(rho_s, rho_t, bmax, float(np.linalg.norm(x)))
        err = abs(exact - model(x))
        worst = max(worst, err / bound)
        assert err <= bound, (err, bound)
        # the information the library would hand over is this quadratic form in xi itself
        Lam = I.information_from_icp(JtJ, T, 1.0)
        assert abs(float(xi @ Lam @ xi) - float(x @ JtJ @ x)) <= 1e-12 * float(x @ JtJ @ x)
        miss_inv.append(abs(exact - model(Adi @ xi)) / bound)
        miss_tr.append(abs(exact - model(Ad.T @ xi)) / bound)
    print("frame: worst error / bound %.3g; misses in bounds, least and median of 20: Ad(T^-1) %.3g, %.3g; Ad^T %.3g, %.3g"
          % (worst, min(miss_inv), np.median(miss_inv), min(miss_tr), np.median(miss_tr)))
    # second order against third: either wrong map is outside the bound for every one of the 20 steps (how far depends
    # on the step's direction), and by more than a decade for most
    assert min(miss_inv) > 1.0 and min(miss_tr) > 1.0
    assert np.median(miss_inv) > 10.0 and np.median(miss_tr) > 10.0


def test_inverse_edge_takes_the_normal_matrix_as_it_is():
    """An edge entered as Z = T^-1 (from the source's pose): (T^-1 Exp(xi))^-1 = Exp(-xi) T is ICP's own left step
    x = -xi, so JtJ is that edge's right-frame information without any adjoint.  Same bound, with the moved points'
    extent in E2 (the step acts on T p)."""
    p, q, nrm, T = corner_pair()
    JtJ, Jtb, bb, moved, b = normal_equations(T, p, q, nrm)
    rho_t, bmax = np.linalg.norm(moved, axis=1).max(), np.abs(b).max()
    Ti = R.inverse(T)
    for xi in _xis(seed=6):
        exact = float(np.sum(residuals(R.inverse(Ti @ R.se3_exp(xi)), p, q, nrm) ** 2))
        x = -xi
        err = abs(exact - (bb - 2.0 * float(x @ Jtb) + float(x @ JtJ @ x)))
        assert err <= third_order_bound(rho_t, rho_t, bmax, XI_NORM), err
    assert np.array_equal(I.information_from_icp(JtJ, np.eye(4), 1.0), np.triu(JtJ) + np.triu(JtJ, 1).T)


def _random_spd(rng, cond):
    Q = np.linalg.qr(rng.normal(size=(6, 6)))[0]
    d = np.exp(rng.uniform(0.0, math.log(cond), 6))
    d[0], d[5] = 1.0, cond
    A = (Q * (d * rng.uniform(1.0, 1e4))) @ Q.T
    return 0.5 * (A + A.T)


@pytest.mark.parametrize("cond", [1.0, 1e3, 1e6])
def test_whitening_is_the_quadratic_form(cond):
    """||R r||^2 = r^T L r.  The Cholesky's backward error is at most 7 ulp of |R^T| |R| entry by entry, forming R r and
    the two quadratic forms some 20 more, and |R^T| |R|_ab <= sqrt(L_aa L_bb): 50 ulp of (sum |r_a| sqrt(L_aa))^2."""
    rng = np.random.default_rng(int(cond) + 3)
    for _ in range(20):
        A = _random_spd(rng, cond)
        U = I.cholesky_upper(A)
        assert np.array_equal(U, np.triu(U)) and (np.diag(U) > 0).all()
        r = rng.normal(size=6)
        tol = 50.0 * np.finfo(float).eps * float(np.sum(np.abs(r) * np.sqrt(np.diag(A)))) ** 2
        assert abs(float(np.sum((U @ r) ** 2)) - float(r @ A @ r)) <= tol


def test_refusals_of_the_restatement():
    A = _random_spd(np.random.default_rng(1), 100.0)
    for bad in (np.nan, np.inf):
        B = A.copy()
        B[2, 3] = bad
        with pytest.raises(R.PoseGraphError):
            I.cholesky_upper(B)
    B = A.copy()
    B[0, 1] += 1e-3 * math.sqrt(A[0, 0] * A[1, 1])
    with pytest.raises(R.PoseGraphError):
        I.cholesky_upper(B)
    with pytest.raises(R.PoseGraphError):
        I.cholesky_upper(-A)
    with pytest.raises(R.PoseGraphError):
        I.cholesky_upper(np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 0.0]))
    g = I.PoseGraph()
    g.add_prior(0, np.eye(4))
    with pytest.raises(R.PoseGraphError):
        g.add_odometry_information(0, 1, np.eye(4), -A)
    assert g.size() == 1 and len(g.factors) == 1 and not g.info_R
    for args in ((0.0, 0, 0), (-1.0, 0, 0), (np.nan, 0, 0), (np.inf, 0, 0), (1.0, -1.0, 0), (1.0, 0, np.nan), (1.0, np.inf, 0)):
        with pytest.raises(R.PoseGraphError):
            I.information_from_icp(A, np.eye(4), *args)


def as_information(ops, cfg=None):
    """Every between factor of `ops` as an information factor with L = diag(1 / sigma^2) of the sigmas it had."""
    cfg = cfg or R.PoseGraphConfig()
    out = []
    for op in ops:
        if op[0] == "odom":
            s = 1.0 + 10.0 * op[4]
            sig = np.array([cfg.odom_rotation_sigma * s] * 3 + [cfg.odom_translation_sigma * s] * 3)
            out.append(("odom_info", op[1], op[2], op[3], np.diag(1.0 / sig ** 2)))
        elif op[0] == "loop":
            sig = np.array([cfg.loop_rotation_sigma] * 3 + [cfg.loop_translation_sigma] * 3)
            out.append(("loop_info", op[1], op[2], op[3], np.diag(1.0 / sig ** 2)))
        else:
            out.append(op)
    return out


@pytest.mark.parametrize("name", ["chain", "ring"])
def test_diagonal_information_is_the_diagonal_model(name):
    """L = diag(1 / sigma^2) on every edge against pose_graph_ref's own run, by the rule of tests/test_gpu_pose_graph.py's
    run_case: same steps, trials and stop; poses within 10x the diagonal run's COLAMD / NATURAL spread (at least
    1e-12 (1 + |t|)); the error history likewise."""
    ops = chain_ops(70, seed=70) if name == "chain" else ring_ops(120, 6, [(5, 110), (30, 100), (63, 64)])
    ref = R.PoseGraph()
    I.apply(ref, ops)
    assert ref.optimize("COLAMD")
    a, sa = np.stack(ref.get_all_poses()), ref.stats
    assert ref.optimize("NATURAL")
    b, sb = np.stack(ref.get_all_poses()), ref.stats
    assert sa.min_margin > 1e-6
    g = I.PoseGraph()
    I.apply(g, as_information(ops))
    assert len(g.info_R) == len(ops) - sum(op[0] == "prior" for op in ops)
    assert g.optimize("COLAMD")
    got, st = np.stack(g.get_all_poses()), g.stats
    assert (st.iterations, st.inner_trials, st.stop_reason) == (sa.iterations, sa.inner_trials, sa.stop_reason)
    tol = np.maximum(10 * np.abs(a - b).reshape(len(a), -1).max(axis=1), 1e-12 * (1 + np.linalg.norm(a[:, :3, 3], axis=1)))
    assert (np.abs(got - a).reshape(len(a), -1).max(axis=1) <= tol).all()
    htol = np.maximum(10 * np.abs(np.array(sa.history) - sb.history), 1e-12 * (1 + np.abs(sa.history)))
    assert (np.abs(np.array(st.history) - sa.history) <= htol).all()


def test_information_edges_beat_isotropic_sigmas_on_a_corridor_ring():
    """The ring of DESIGN 7.13: 200 poses, odometry looser along track than across it on every edge and all but blind
    along track on twenty edges, four accurate closures.  The graph that is told each edge's inverse covariance must have
    a strictly lower ATE than the one that weighs every edge by the config's isotropic sigmas, on every committed seed."""
    assert len(I.RING_SEEDS) >= 8
    assert I.RING_ALONG_CORRIDOR > 10 * I.RING_CROSS and I.RING_ALONG > 3 * I.RING_CROSS
    for seed in I.RING_SEEDS:
        iso, info = I.ring_ates(seed)
        print("seed %d: ATE isotropic %.4f m, information %.4f m" % (seed, iso, info))
        assert info < iso, (seed, iso, info)
