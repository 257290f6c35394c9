"""scripts/pose_graph_ref.py -- the CPU restatement of the reference's GTSAM pose graph (core/pose_graph.cpp) that
tests/test_gpu_pose_graph.py holds the device optimiser to -- checked on its own: the SE(3) maps, every Jacobian
against central differences, closed forms, the reference's bookkeeping quirks and a drift case.  Runs on the CPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import pose_graph_ref as P  # noqa: E402
from lidar_slam_from_scratch_amd import synth  # noqa: E402


def _xi(rng, theta, vscale=1.0):
    w = rng.normal(size=3)
    w *= theta / np.linalg.norm(w)
    return np.r_[w, vscale * rng.normal(size=3)]


THETAS = [0.0, 1e-12, 1e-9, 1e-6, 1e-3, 0.0999, 0.1, 0.1001, 0.7, 2.0, 3.0, np.pi - 1e-3, np.pi - 1e-7]


@pytest.mark.parametrize("theta", THETAS)
def test_exp_log_round_trip(theta):
    rng = np.random.default_rng(int(theta * 1e6) % 1000 + 1)
    for _ in range(5):
        xi = _xi(rng, theta)
        T = P.se3_exp(xi)
        assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-15
        back = P.se3_log(T)
        assert np.abs(back - xi).max() <= 4e-15 * max(1.0, 1.0 / max(np.pi - theta, 1e-3) * 1e-3 + 1.0), (theta, back - xi)
        # and the other way: Exp(Log(T)) == T
        assert np.abs(P.se3_exp(back) - T).max() < 4e-15


def test_log_of_identity_is_exactly_zero():
    assert (P.se3_log(np.eye(4)) == 0).all()
    J = P.se3_jr_inv(np.zeros(6))
    assert (J == np.eye(6)).all()


@pytest.mark.parametrize("theta", [0.0, 1e-8, 0.05, 0.3, 1.5, 3.0])
def test_exp_matches_synth_rodrigues(theta):
    rng = np.random.default_rng(3)
    w = _xi(rng, theta)[:3]
    assert np.abs(P.so3_exp(w) - synth.rotvec_to_matrix(w)).max() < 2e-16 * 8


def _num_jac(f, x, h=1e-6):
    J = np.zeros((6, 6))
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        J[:, k] = (f(x + e) - f(x - e)) / (2 * h)
    return J


@pytest.mark.parametrize("theta", [0.0, 1e-7, 0.05, 0.0999, 0.1001, 0.6, 2.5])
def test_jr_inv_against_central_differences(theta):
    rng = np.random.default_rng(11)
    xi = _xi(rng, theta, 2.0)
    T = P.se3_exp(xi)
    num = _num_jac(lambda d: P.se3_log(T @ P.se3_exp(d)), np.zeros(6))
    assert np.abs(num - P.se3_jr_inv(xi)).max() < 1e-8


def _rand_pose(rng, theta=1.0, t=3.0):
    return P.se3_exp(_xi(rng, theta * rng.uniform(), t))


@pytest.mark.parametrize("seed", range(4))
def test_factor_jacobians_against_central_differences(seed):
    rng = np.random.default_rng(seed)
    X = np.stack([_rand_pose(rng), _rand_pose(rng)])
    Zb, Zp = _rand_pose(rng), _rand_pose(rng)
    kind, fi, fj = np.array([1, 0]), np.array([0, 1]), np.array([1, 0])
    Z = np.stack([Zb, Zp])
    r, Ji, Jj = P.factor_residuals(kind, fi, fj, Z, X)

    def res(node, f):
        def g(d):
            Xd = X.copy()
            Xd[node] = X[node] @ P.se3_exp(d)
            return P.factor_residuals(kind, fi, fj, Z, Xd)[0][f]
        return g

    assert np.abs(_num_jac(res(0, 0), np.zeros(6)) - Ji[0]).max() < 1e-7     # between, d/dxi_i
    assert np.abs(_num_jac(res(1, 0), np.zeros(6)) - Jj[0]).max() < 1e-7     # between, d/dxi_j
    assert np.abs(_num_jac(res(1, 1), np.zeros(6)) - Ji[1]).max() < 1e-7     # prior
    # the residuals themselves
    assert np.abs(r[0] - P.se3_log(np.linalg.inv(Zb) @ np.linalg.inv(X[0]) @ X[1])).max() < 1e-13
    assert np.abs(r[1] - P.se3_log(np.linalg.inv(Zp) @ X[1])).max() < 1e-13


def test_prior_plus_one_between_closed_form():
    rng = np.random.default_rng(5)
    Pp, Z = _rand_pose(rng), _rand_pose(rng)
    g = P.PoseGraph()
    g.add_prior(0, Pp)
    g.add_odometry_factor(0, 1, Z)
    assert g.optimize()
    assert g.final_error < 1e-25
    assert np.abs(g.get_pose(1) - Pp @ Z).max() < 1e-14
    assert np.abs(g.get_pose(0) - Pp).max() < 1e-15
    # identity prior: exactly zero error, no iteration (defaultOptimize's errorTol test)
    g = P.PoseGraph()
    g.add_prior(0, np.eye(4))
    g.add_odometry_factor(0, 1, np.eye(4))
    assert g.optimize() and g.final_error == 0.0 and g.iterations == 0
    assert g.stats.stop_reason == P.STOP_ZERO_ERROR


def _circle(n, radius=30.0):
    out = []
    for k in range(n):
        a = 2 * np.pi * k / n
        out.append(synth.make_transform([0.0, 0.0, a], [radius * np.cos(a), radius * np.sin(a), 0.3 * np.sin(3 * a)]))
    return out


def test_ground_truth_measurements_converge_to_truth():
    rng = np.random.default_rng(2)
    gt = _circle(40)
    g = P.PoseGraph()
    g.add_prior(0, gt[0])
    for k in range(39):
        g.add_odometry_factor(k, k + 1, np.linalg.inv(gt[k]) @ gt[k + 1])
    g.add_loop_closure(0, 39, np.linalg.inv(gt[0]) @ gt[39])
    # start away from the truth: overwrite the chained estimates with perturbed ones
    for k in range(1, 40):
        g.initial[k] = gt[k] @ P.se3_exp(np.r_[rng.normal(0, 0.02, 3), rng.normal(0, 0.3, 3)])
    assert g.optimize()
    for k in range(40):
        assert np.abs(g.get_pose(k) - gt[k]).max() < 1e-9
    assert g.final_error < 1e-15


def test_bookkeeping_quirks():
    rng = np.random.default_rng(8)
    A, B, C = _rand_pose(rng), _rand_pose(rng), _rand_pose(rng)
    g = P.PoseGraph()
    assert not g.optimize()                                   # empty graph (pose_graph.cpp:148-150)
    g.add_prior(0, A)
    g.add_odometry_factor(0, 1, B)                            # chained: X1 = X0 * Z
    g.add_odometry_factor(1, 2, C)
    assert np.abs(g.get_pose(2) - A @ B @ C).max() < 1e-13
    g.add_odometry_factor(0, 2, B)                            # existing estimate kept
    assert np.abs(g.get_pose(2) - A @ B @ C).max() < 1e-13
    assert g.optimize()
    opt = g.get_all_poses()
    g.add_prior(0, B)                                         # addPrior leaves optimized_ set
    assert g.optimized and all((a == b).all() for a, b in zip(g.get_all_poses(), opt))
    assert g.get_pose(0) is not None and (g.initial[0] == A).all()      # the estimate stays the first one
    g.add_loop_closure(0, 2, C)                               # clears optimized_: initial estimates again
    assert not g.optimized and (g.get_pose(2) == g.initial[2]).all()
    assert g.loop_closure_count() == 1
    # optimize restarts from the initial estimates: twice in a row gives the same poses
    g.optimize()
    first = np.stack(g.get_all_poses())
    g.optimize()
    assert (np.stack(g.get_all_poses()) == first).all()
    # getAllPoses skips gaps; getPose of a gap fails
    g.add_odometry_factor(2, 5, B)
    assert g.size() == 6 and len(g.get_all_poses()) == 4
    with pytest.raises(P.PoseGraphError):
        g.get_pose(3)
    # a factor from a pose with no estimate to one without is refused and changes nothing
    nf = len(g.factors)
    with pytest.raises(P.PoseGraphError):
        g.add_odometry_factor(7, 8, B)
    assert len(g.factors) == nf and g.size() == 6
    with pytest.raises(P.PoseGraphError):
        g.add_loop_closure(3, 3, B)
    bad = B.copy()
    bad[0, 3] = np.nan
    with pytest.raises(P.PoseGraphError):
        g.add_prior(1, bad)
    # a loop closure onto a pose with no estimate: optimize returns false (the reference's catch)
    g.add_loop_closure(0, 9, B)
    assert not g.optimize()


def test_sigma_scale_of_fitness():
    g = P.PoseGraph()
    g.add_prior(0, np.eye(4))
    g.add_odometry_factor(0, 1, np.eye(4), fitness=0.25)
    s = g.factors[1][4]
    assert np.allclose(s, [0.01 * 3.5] * 3 + [0.05 * 3.5] * 3, rtol=0, atol=1e-17)
    g.add_loop_closure(0, 1, np.eye(4))
    assert (g.factors[2][4] == [0.005] * 3 + [0.025] * 3).all()
    assert (g.factors[0][4] == [0.001] * 6).all()


def _ate(poses, gt):
    return float(np.sqrt(np.mean([np.sum((a[:3, 3] - b[:3, 3]) ** 2) for a, b in zip(poses, gt)])))


def test_drift_case_loop_closures_cut_ate():
    rng = np.random.default_rng(1)
    n = 200
    gt = _circle(n)
    g = P.PoseGraph()
    g.add_prior(0, gt[0])
    for k in range(n - 1):
        noise = P.se3_exp(np.r_[rng.normal(0, 0.004, 3), rng.normal(0, 0.03, 3)])
        g.add_odometry_factor(k, k + 1, np.linalg.inv(gt[k]) @ gt[k + 1] @ noise)
    for i, j in [(0, 190), (0, 195), (5, 199), (50, 150)]:
        g.add_loop_closure(i, j, np.linalg.inv(gt[i]) @ gt[j])
    odo = g.get_all_poses()
    assert g.optimize()
    assert _ate(g.get_all_poses(), gt) <= _ate(odo, gt) / 3.0
    # the two orderings agree to rounding
    a = np.stack(g.get_all_poses())
    g.optimize("NATURAL")
    assert np.abs(np.stack(g.get_all_poses()) - a).max() < 1e-10
    # and so does the dense Cholesky of the same matrices, step for step
    it = (g.stats.iterations, g.stats.inner_trials)
    g.optimize("DENSE")
    assert np.abs(np.stack(g.get_all_poses()) - a).max() < 1e-10 and (g.stats.iterations, g.stats.inner_trials) == it


def rotational_drift_graph(n=60, drift=0.1):
    """A ring whose odometry over-turns by `drift` rad a step, closed twice: LM rejects steps and raises lambda."""
    g = P.PoseGraph()
    g.add_prior(0, np.eye(4))
    a = 2 * np.pi / n
    Z = synth.make_transform([0, 0, a + drift], [2.0, 0, 0])
    for k in range(n - 1):
        g.add_odometry_factor(k, k + 1, Z)
    g.add_loop_closure(0, n - 1, synth.make_transform([0, 0, -a], [-2.0, 0, 0]))
    g.add_loop_closure(0, n // 2, synth.make_transform([0, 0, np.pi], [0, 2 * n / np.pi, 0]))
    return g


def test_rejected_steps_raise_lambda():
    g = rotational_drift_graph()
    assert g.optimize()
    assert g.stats.inner_trials > g.stats.iterations + 1
    assert g.stats.stop_reason == P.STOP_RELATIVE
