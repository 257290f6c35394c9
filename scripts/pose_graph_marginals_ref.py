#!/usr/bin/env python3
"""CPU restatement of the pose graph's covariances (csrc/pose_graph_marginals.h, pose_graph_marginals_host.h; DESIGN
7.14), the yardstick of icpmi_pose_graph_marginals / _relative_covariance / _closure_distance.

H is the Gauss-Newton matrix of the whole graph at given poses: pose_graph_ref's whitened Jacobians (through the
`linearize` hooks of pose_graph_loss_ref / pose_graph_info_ref where the graph has a loop loss or information edges)
summed into normal equations, no damping.  The joint marginal covariance of q poses is the blocks (H^-1)[a, b], tangent
order (omega, v), right perturbation X Exp(xi).  The selected columns are solved three ways -- sparse LU under COLAMD
and under NATURAL ordering, dense Cholesky -- and the spread of the three is the yardstick's own rounding.

    relative covariance   Sigma_rel = J Sigma J^T, J = [-Ad(X_j^-1 X_i), I]: the tangent of X_i^-1 X_j to first order
    closure distance      e = Log(Z^-1 X_i^-1 X_j), d^2 = e^T (Sigma_rel + Sigma_edge)^-1 e, chi-squared with 6 degrees
                          of freedom for a true closure

Run as a program: the closure distances of pose_graph_loss_ref.false_closure_ring against the chain optimised without
any closure (the table of DESIGN 7.14)."""
import os
import sys

import numpy as np
import scipy.linalg as sla
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_ref as R  # noqa: E402
import pose_graph_loss_ref as L  # noqa: E402
import pose_graph_info_ref as I  # noqa: E402

ORDERINGS = ("COLAMD", "NATURAL", "DENSE")
CHI2_6_99 = 16.811893829770927      # the 0.99 quantile of chi-squared with 6 degrees of freedom
CHI2_6_999 = 22.457744484825323     # the 0.999 quantile


def hessian(g, poses=None):
    """-> (keys, H) with H the sparse 6n x 6n Gauss-Newton matrix of graph g (a PoseGraph of pose_graph_ref, _loss_ref or
    _info_ref) at `poses` (index -> 4x4 or a list over the keys; default the graph's current values), loss weights and
    information edges as the optimiser applies them."""
    keys, kind, fi, fj, Z, inv_sigma, X0 = g.arrays()
    if poses is None:
        poses = g._values()
    X = np.stack([np.asarray(poses[k], dtype=np.float64) for k in keys] if isinstance(poses, dict) else list(poses))
    assert X.shape == (len(keys), 4, 4)
    loops = getattr(g, "loop_factors", [])
    loss = bool(loops) and getattr(g, "loss_kind", L.LOSS_NONE) != L.LOSS_NONE
    if getattr(g, "info_R", None):
        slot, Rs = g._slots()
        args = (g._is_loop(), g.loss_kind, g.loss_scale) if loss else ()
        linearize = I.info_linearize(slot, Rs, *args)
    elif loss:
        linearize = L.loss_linearize(g._is_loop(), g.loss_kind, g.loss_scale)
    else:
        linearize = R._linearize
    rw, Ai, Aj = linearize(kind, fi, fj, Z, inv_sigma, X)
    H, _ = R._normal_equations(len(keys), kind, fi, fj, rw, Ai, Aj)
    return keys, H


def selected_columns(H, nodes, ordering):
    """Columns of H^-1 that belong to the compact nodes `nodes` (6 each), by one of the three solves."""
    n = H.shape[0]
    E = np.zeros((n, 6 * len(nodes)))
    for a, v in enumerate(nodes):
        E[6 * v:6 * v + 6, 6 * a:6 * a + 6] = np.eye(6)
    if ordering == "DENSE":
        Lc = np.linalg.cholesky(H.toarray())
        return sla.solve_triangular(Lc, sla.solve_triangular(Lc, E, lower=True), lower=True, trans="T")
    lu = spla.splu(H.tocsc(), permc_spec=ordering, diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    piv = lu.U.diagonal()
    if not np.all(np.isfinite(piv)) or np.any(piv <= 0.0):
        raise np.linalg.LinAlgError("non-positive pivot: the graph has no covariance")
    return lu.solve(E)


def joint_marginal(H, keys, indices, ordering="COLAMD"):
    """-> the (6q, 6q) joint marginal covariance of pose indices `indices`."""
    pos = {k: p for p, k in enumerate(keys)}
    nodes = [pos[int(i)] for i in indices]
    if len(set(nodes)) != len(nodes) or not nodes:
        raise R.PoseGraphError("a covariance query names distinct poses")
    X = selected_columns(H, nodes, ordering)
    rows = np.concatenate([np.arange(6 * v, 6 * v + 6) for v in nodes])
    return X[rows]


def joint_marginals_three(H, keys, indices):
    """-> (COLAMD's answer, the largest normalised difference of the other two solves from it): |dSigma_ab| /
    sqrt(Sigma_aa Sigma_bb), the error measure of the device tests."""
    a = joint_marginal(H, keys, indices, "COLAMD")
    spread = 0.0
    for o in ORDERINGS[1:]:
        spread = max(spread, normalised_error(joint_marginal(H, keys, indices, o), a))
    return a, spread


def normalised_error(got, ref):
    d = np.sqrt(np.abs(np.diag(ref)))
    return float(np.max(np.abs(got - ref) / np.outer(d, d)))


def relative_covariance(Xi, Xj, joint):
    """joint: 12 x 12 of (i, j).  -> 6 x 6."""
    J = np.hstack([-R.adjoint(R.inverse(Xj) @ Xi), np.eye(6)])
    return J @ joint @ J.T


def closure_distance(Xi, Xj, Z, rel_cov, edge_cov):
    e = R.se3_log(R.inverse(Z) @ (R.inverse(Xi) @ Xj))
    M = np.asarray(rel_cov) + np.asarray(edge_cov)
    Lc = np.linalg.cholesky(M)               # raises LinAlgError where the sum is not positive definite
    y = sla.solve_triangular(Lc, e, lower=True)
    return float(y @ y)


def loop_edge_covariance(cfg):
    return np.diag([cfg.loop_rotation_sigma ** 2] * 3 + [cfg.loop_translation_sigma ** 2] * 3)


def ring_distances(seed=1):
    """-> [(i, j, d2, is_false)] for every closure of false_closure_ring(seed), each against the odometry chain
    optimised without any closure (what a gate sees before the first one enters)."""
    ops = L.false_closure_ring(seed)
    g = L.PoseGraph()
    L.apply(g, [op for op in ops if op[0] != "loop"])
    assert g.optimize()
    keys, H = hessian(g)
    X = g.optimized_values
    Se = loop_edge_covariance(g.config)
    loops = [op for op in ops if op[0] == "loop"]
    out = []
    for n, (_, i, j, Z) in enumerate(loops):
        S = relative_covariance(X[i], X[j], joint_marginal(H, keys, [i, j]))
        out.append((i, j, closure_distance(X[i], X[j], Z, S, Se), n == len(loops) - 1))
    return out


def main():
    print("chi-squared, 6 degrees of freedom: 0.99 -> %.2f, 0.999 -> %.2f" % (CHI2_6_99, CHI2_6_999))
    print("| closure | d^2 | |")
    print("|---|---|---|")
    for i, j, d2, false in ring_distances():
        print("| (%d, %d) | %.4g | %s |" % (i, j, d2, "false" if false else "true"))


if __name__ == "__main__":
    main()
