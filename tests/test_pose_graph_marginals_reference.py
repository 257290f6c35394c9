"""The CPU restatement of the pose graph's covariances (scripts/pose_graph_marginals_ref.py) on cases with a known
answer, and the fixture behind the device tests' floor (scripts/make_marginals_case.py).  No GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_marginals_case as mk  # noqa: E402
import pose_graph_loss_ref as L  # noqa: E402
import pose_graph_marginals_ref as M  # noqa: E402
import pose_graph_ref as R  # noqa: E402
import test_gpu_pose_graph as G  # noqa: E402

CASE = np.load(os.path.join(ROOT, "tests", "golden", "pose_graph_marginals_case.npz"))


def _chain_one_prior(n, seed):
    g = R.PoseGraph()
    G.apply(g, G.chain_ops(n, seed)[:-1])          # without its second prior
    assert g.optimize()
    return g


def test_a_pose_with_only_a_prior_has_the_priors_covariance():
    g = R.PoseGraph()
    g.add_prior(0, np.eye(4))
    keys, H = M.hessian(g)
    for o in M.ORDERINGS:
        S = M.joint_marginal(H, keys, [0], o)
        assert np.allclose(S, 1e-6 * np.eye(6), rtol=1e-12, atol=1e-20)
    g = _chain_one_prior(130, 130)
    keys, H = M.hessian(g)
    S = M.joint_marginal(H, keys, [0])
    print("pose 0 of chain130:", np.diag(S))
    assert np.allclose(np.diag(S), 1e-6, rtol=1e-9)


def test_adjacent_poses_of_a_pure_chain_are_apart_by_the_edges_noise():
    ops = G.chain_ops(130, 130)[:-1]
    g = _chain_one_prior(130, 130)
    keys, H = M.hessian(g)
    X = g.optimized_values
    for k in (0, 1, 62, 63, 64, 128):
        op = [o for o in ops if o[0] == "odom" and o[1] == k][0]
        scale = 1.0 + 10.0 * op[4]
        want = np.diag([(0.01 * scale) ** 2] * 3 + [(0.05 * scale) ** 2] * 3)
        S = M.relative_covariance(X[k], X[k + 1], M.joint_marginal(H, keys, [k, k + 1]))
        d = np.sqrt(np.diag(want))
        err = np.abs(S - want) / np.outer(d, d)
        print("edge (%d, %d): worst normalised deviation %.3g" % (k, k + 1, err.max()))
        # a pure chain at its optimum has zero residuals up to the optimiser's stopping error, where Jr^-1 = I and the
        # relative covariance is the edge's own; what is left is the joint covariance's cancellation: Sigma grows
        # along the chain while the difference stays sigma^2, so the relative rounding is eps * |J||Sigma||J^T| / sigma^2
        Ja = np.abs(np.hstack([R.adjoint(R.inverse(X[k + 1]) @ X[k]), np.eye(6)]))
        joint = M.joint_marginal(H, keys, [k, k + 1])
        cancel = (Ja @ np.abs(joint) @ Ja.T) / np.outer(d, d)
        assert (err <= 1e-9 + 1e3 * np.finfo(float).eps * cancel).all()


def test_the_three_solves_agree():
    g = L.PoseGraph()
    L.apply(g, L.false_closure_ring(1))
    g.set_loop_loss(L.LOSS_CAUCHY, 3.0)
    assert g.optimize()
    keys, H = M.hessian(g)
    a, spread = M.joint_marginals_three(H, keys, [30, 150, 199])
    print("spread of the three solves on the ring under Cauchy: %.3g" % spread)
    assert spread < 1e-8 and np.allclose(a, a.T, rtol=0, atol=1e-8 * np.abs(a).max())


def test_false_closure_is_far_and_true_ones_pass():
    """The gate is chi-squared's, not the data's: the 0.999 quantile at 6 degrees of freedom."""
    rows = M.ring_distances(1)
    for i, j, d2, false in rows:
        print("closure (%d, %d) d2 %.4g %s" % (i, j, d2, "false" if false else "true"))
    assert [r[3] for r in rows] == [False] * (len(rows) - 1) + [True]
    assert all(d2 <= M.CHI2_6_999 for _, _, d2, false in rows if not false)
    assert rows[-1][2] > M.CHI2_6_999 and rows[-1][2] > 5.0 * max(r[2] for r in rows[:-1])


def test_loss_weights_enter_the_matrix():
    """Under Cauchy the refused closure carries almost no information: the covariance of its far end is the clean
    graph's within a part in a hundred, while with the Gaussian model the false edge tightens it visibly."""
    ops = L.false_closure_ring(1)
    clean = L.PoseGraph()
    L.apply(clean, ops[:-1])
    assert clean.optimize()
    keys, Hc = M.hessian(clean)
    Sc = M.joint_marginal(Hc, keys, [150])
    robust = L.PoseGraph()
    robust.set_loop_loss(L.LOSS_CAUCHY, 3.0)
    L.apply(robust, ops)
    assert robust.optimize()
    _, Hr = M.hessian(robust)
    Sr = M.joint_marginal(Hr, keys, [150])
    assert np.abs(np.diag(Sr) / np.diag(Sc) - 1.0).max() < 1e-2


def test_fixture_floor_is_the_restatements_own_error():
    """The floor's source: the restatement against the 50-digit inverse stored with the fixture."""
    g = mk.graph_of(CASE["kind"], CASE["fi"], CASE["fj"], CASE["Z"], CASE["fitness"])
    keys, H = M.hessian(g, list(CASE["poses"]))
    assert np.allclose(H.toarray(), CASE["H"], rtol=1e-13, atol=0.0)
    n = len(keys)
    worst = max(M.normalised_error(M.joint_marginal(H, keys, list(range(n)), o), CASE["inverse"]) for o in M.ORDERINGS)
    stored = float(CASE["restatement_error"])
    print("restatement against the 50-digit inverse: %.3g (stored %.3g)" % (worst, stored))
    assert worst <= 2.0 * stored and 0.0 < stored < 1e-12
