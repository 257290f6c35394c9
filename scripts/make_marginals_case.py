#!/usr/bin/env python3
"""Writes tests/golden/pose_graph_marginals_case.npz: a small pose graph (20 tumbling poses, two loops), its Gauss-Newton
matrix H at the restatement's optimum, H^-1 from a 50-digit inversion (mpmath) rounded to fp64, and the worst error of
scripts/pose_graph_marginals_ref.py's three solves against it, in the tests' measure |dSigma_ab| / sqrt(Sigma_aa
Sigma_bb).  Eight times that error is the floor of the device tests' bound (tests/test_gpu_pose_graph_marginals.py):
what fp64 leaves of a covariance on a well-conditioned graph however it is solved.

The graph is rebuilt from the stored factors by the tests, so the fixture does not depend on a random generator's
stream."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_graph_ref as R  # noqa: E402
import pose_graph_marginals_ref as M  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "pose_graph_marginals_case.npz")
N, LOOPS, SEED = 20, ((2, 15), (6, 18)), 2014


def case_ops():
    rng = np.random.default_rng(SEED)
    gt = [np.eye(4)]
    for _ in range(N - 1):
        gt.append(gt[-1] @ R.se3_exp(np.r_[rng.normal(0, 0.3, 3), 1.0 + rng.normal(0, 0.1), rng.normal(0, 0.2, 2)]))

    def noise(rs, ts):
        return R.se3_exp(np.r_[rng.normal(0, rs, 3), rng.normal(0, ts, 3)])

    ops = [("prior", 0, gt[0])]
    ops += [("odom", k, k + 1, np.linalg.inv(gt[k]) @ gt[k + 1] @ noise(0.004, 0.03), 0.0) for k in range(N - 1)]
    ops += [("loop", i, j, np.linalg.inv(gt[i]) @ gt[j] @ noise(0.001, 0.01)) for i, j in LOOPS]
    return ops


def graph_of(kind, fi, fj, Z, fitness):
    """The restatement's graph from the fixture's arrays (kind 0 prior, 1 odometry, 2 loop closure)."""
    g = R.PoseGraph()
    for k, i, j, z, f in zip(kind, fi, fj, Z, fitness):
        if k == 0:
            g.add_prior(int(i), z)
        elif k == 1:
            g.add_odometry_factor(int(i), int(j), z, float(f))
        else:
            g.add_loop_closure(int(i), int(j), z)
    return g


def main():
    ops = case_ops()
    kind = np.array([{"prior": 0, "odom": 1, "loop": 2}[op[0]] for op in ops])
    fi = np.array([op[1] for op in ops])
    fj = np.array([op[2] if op[0] != "prior" else -1 for op in ops])
    Z = np.stack([op[2] if op[0] == "prior" else op[3] for op in ops])
    fitness = np.array([op[4] if op[0] == "odom" else 0.0 for op in ops])
    g = graph_of(kind, fi, fj, Z, fitness)
    assert g.optimize()
    import mpmath
    X = np.stack(g.get_all_poses())
    keys, H = M.hessian(g)
    Hd = H.toarray()
    mpmath.mp.dps = 50
    inv = mpmath.matrix(Hd.tolist()) ** -1
    exact = np.array([[float(inv[r, c]) for c in range(6 * N)] for r in range(6 * N)])
    worst = 0.0
    for o in M.ORDERINGS:
        worst = max(worst, M.normalised_error(M.joint_marginal(H, keys, list(range(N)), o), exact))
    print("condition %.3g, the restatement's worst error against the 50-digit inverse: %.3g" % (np.linalg.cond(Hd), worst))
    np.savez_compressed(OUT, kind=kind, fi=fi, fj=fj, Z=Z, fitness=fitness, poses=X, H=Hd, inverse=exact,
                        restatement_error=np.float64(worst))


if __name__ == "__main__":
    main()
