#!/usr/bin/env python3
"""CPU restatement of a robust loss on the pose graph's loop-closure edges: GTSAM 4.1+ noiseModel::Robust over the loop
factors' diagonal model, restated from the source as published (there is no GTSAM build to check against), the
yardstick of csrc/pose_graph_loss.h.

The setting is the graph's, not a factor's: it applies to every factor added by add_loop_closure, past and future, at
the next optimize().  Priors and odometry factors are never touched.  Per loop factor rw = r / sigma and
d = sqrt(sum rw_a^2), `scale` k in whitened units (sigmas):
    HUBER (1)          w = d <= k ? 1 : k / d              rho = d <= k ? 0.5 d^2 : k (d - 0.5 k)
    CAUCHY (2)         s = k k,  w = s / (s + d^2)         rho = 0.5 s log1p(d^2 / s)
    GEMAN_MCCLURE (3)  s = k k,  q = s / (s + d^2), w = q q   rho = 0.5 s d^2 / (s + d^2)
No form divides by d except Huber's outer branch, where d > k > 0.
Linearisation (Robust::WhitenSystem): A_i, A_j and rw of a loop factor are multiplied by sqrt(w) (q itself for
Geman-McClure, sqrt() for the other two); H, g and the linearised error are formed from the scaled values.
Error (NoiseModelFactor::error -> Robust::loss): a loop factor contributes rho(d), every other factor 0.5 d^2, for the
initial error, every trial's candidate error, the history and final_error.  The LM policy is pose_graph_ref's,
untouched, through its two hooks.

Run as a program: the table of DESIGN 7.12 (one false closure on a two-lap ring)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_ref as R  # noqa: E402

LOSS_NONE, LOSS_HUBER, LOSS_CAUCHY, LOSS_GEMAN_MCCLURE = range(4)
LOSS_NAMES = {LOSS_NONE: "Gaussian", LOSS_HUBER: "Huber", LOSS_CAUCHY: "Cauchy", LOSS_GEMAN_MCCLURE: "Geman-McClure"}


def loss_weight_rho(d, kind, k):
    """(w, rho, sqrt(w)) of whitened distances d (array or scalar) under loss `kind` of scale k."""
    d = np.asarray(d, dtype=np.float64)
    d2 = d * d
    if kind == LOSS_NONE:
        w = np.ones_like(d)
        return w, 0.5 * d2, w
    if kind == LOSS_HUBER:
        inner = d <= k
        w = np.where(inner, 1.0, k / np.where(inner, 1.0, d))
        return w, np.where(inner, 0.5 * d2, k * (d - 0.5 * k)), np.sqrt(w)
    s = k * k
    if kind == LOSS_CAUCHY:
        w = s / (s + d2)
        return w, 0.5 * s * np.log1p(d2 / s), np.sqrt(w)
    if kind == LOSS_GEMAN_MCCLURE:
        q = s / (s + d2)
        return q * q, 0.5 * s * d2 / (s + d2), q
    raise R.PoseGraphError("loss kind %r" % (kind,))


class HuberWatch:
    """Smallest |d - k| / k of any Huber loop factor at any linearisation or error evaluation: the branch a rounding
    could flip."""

    def __init__(self):
        self.min_margin = math.inf

    def see(self, d, kind, k):
        if kind == LOSS_HUBER and len(d):
            self.min_margin = min(self.min_margin, float(np.min(np.abs(d - k) / k)))


def _distance(rw):
    return np.sqrt(np.sum(rw * rw, axis=1))


def loss_linearize(is_loop, kind, k, watch=None):
    """The `linearize` hook of pose_graph_ref.levenberg_marquardt: Diagonal::WhitenSystem, then Robust's sqrt(w) on the
    loop factors' rows."""
    def linearize(fkind, fi, fj, Z, inv_sigma, X):
        rw, Ai, Aj = R._linearize(fkind, fi, fj, Z, inv_sigma, X)
        d = _distance(rw[is_loop])
        if watch is not None:
            watch.see(d, kind, k)
        sw = loss_weight_rho(d, kind, k)[2]
        rw[is_loop] = rw[is_loop] * sw[:, None]
        Ai[is_loop] = Ai[is_loop] * sw[:, None, None]
        Aj[is_loop] = Aj[is_loop] * sw[:, None, None]
        return rw, Ai, Aj
    return linearize


def loss_factor_errors(is_loop, kind, k, watch=None):
    """The `errors` hook: rho(d) for a loop factor, 0.5 d^2 for every other."""
    def errors(fkind, fi, fj, Z, inv_sigma, X):
        rw = R.factor_residuals(fkind, fi, fj, Z, X)[0] * inv_sigma
        e = 0.5 * np.sum(rw * rw, axis=1)
        d = _distance(rw[is_loop])
        if watch is not None:
            watch.see(d, kind, k)
        e[is_loop] = loss_weight_rho(d, kind, k)[1]
        return e
    return errors


class PoseGraph(R.PoseGraph):
    """pose_graph_ref.PoseGraph with icpmi_pose_graph_set_loop_loss / _loop_loss / _loop_weights."""

    def __init__(self, config=None):
        super().__init__(config)
        self.loss_kind, self.loss_scale = LOSS_NONE, 0.0
        self.loop_factors = []       # positions in self.factors, in add_loop_closure order

    def set_loop_loss(self, kind, scale=0.0):
        if kind not in (LOSS_NONE, LOSS_HUBER, LOSS_CAUCHY, LOSS_GEMAN_MCCLURE):
            raise R.PoseGraphError("loss kind %r" % (kind,))
        if kind != LOSS_NONE and not (math.isfinite(scale) and scale > 0.0):
            raise R.PoseGraphError("loss scale must be finite and positive")
        new = (int(kind), float(scale) if kind != LOSS_NONE else 0.0)
        if new != (self.loss_kind, self.loss_scale):
            self.loss_kind, self.loss_scale = new
            self.optimized = False

    def loop_loss(self):
        return self.loss_kind, self.loss_scale

    def add_loop_closure(self, i, j, Z):
        super().add_loop_closure(i, j, Z)
        self.loop_factors.append(len(self.factors) - 1)

    def _is_loop(self):
        m = np.zeros(len(self.factors), dtype=bool)
        m[self.loop_factors] = True
        return m

    def optimize(self, ordering="COLAMD"):
        if self.num_poses == 0:
            return False
        a = self.arrays()
        if a is None:
            return False
        keys, kind, fi, fj, Z, inv_sigma, X0 = a
        hooks = {}
        watch = HuberWatch()
        if self.loss_kind != LOSS_NONE and self.loop_factors:
            m = self._is_loop()
            hooks = dict(linearize=loss_linearize(m, self.loss_kind, self.loss_scale, watch),
                         errors=loss_factor_errors(m, self.loss_kind, self.loss_scale, watch))
        X, st = R.levenberg_marquardt(kind, fi, fj, Z, inv_sigma, X0, self.config, ordering, **hooks)
        st.min_margin = min(st.min_margin, watch.min_margin)
        self.optimized_values = {k: X[p] for p, k in enumerate(keys)}
        self.final_error, self.iterations, self.stats = st.final_error, st.iterations, st
        self.optimized = True
        return True

    def loop_distances_at(self, poses):
        """Whitened distance of every loop closure, in add_loop_closure order, at `poses` (index -> 4x4, or the list
        get_all_poses() returns when no index is skipped)."""
        keys, kind, fi, fj, Z, inv_sigma, _ = self.arrays()
        X = np.stack([poses[k] for k in keys])
        lf = np.array(self.loop_factors, dtype=np.int64)
        rw = R.factor_residuals(kind[lf], fi[lf], fj[lf], Z[lf], X)[0] * inv_sigma[lf] if len(lf) else np.zeros((0, 6))
        return _distance(rw)

    def loop_weights(self):
        """(weights, distances) at the optimised values; weights are 1 with the loss off."""
        if not self.optimized:
            raise R.PoseGraphError("no optimised state")
        d = self.loop_distances_at(self.optimized_values)
        return loss_weight_rho(d, self.loss_kind, self.loss_scale)[0], d


# ------------------------------------------------------------------------------------------- the table of DESIGN 7.12

def _transform(rpy, t):
    cr, sr, cp, sp_, cy, sy = math.cos(rpy[0]), math.sin(rpy[0]), math.cos(rpy[1]), math.sin(rpy[1]), \
        math.cos(rpy[2]), math.sin(rpy[2])
    T = np.eye(4)
    T[:3, :3] = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp_], [0, 1, 0], [-sp_, 0, cp]]) \
        @ np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    T[:3, 3] = t
    return T


def false_closure_ring(seed, lap=100, n=None, radius=30.0, true_loops=None, false_loop=(30, 150),
                       make_transform=_transform):
    """A ring of n poses (default two laps of `lap`), drifting odometry, true closures (default (k, k + lap) for
    k = 10, 20, .. lap - 10) and, last, one false closure whose measurement is about identity.  Returns the op list;
    ops[:-1] is the clean graph."""
    rng = np.random.default_rng(seed)
    n = 2 * lap if n is None else n
    if true_loops is None:
        true_loops = [(k, k + lap) for k in range(10, lap, 10)]

    def noise(rs, ts):
        return R.se3_exp(np.r_[rng.normal(0, rs, 3), rng.normal(0, ts, 3)])

    def rel(a, b):
        return np.linalg.inv(a) @ b

    gt = [make_transform([0, 0, 2 * np.pi * k / lap], [radius * np.cos(2 * np.pi * k / lap),
                                                        radius * np.sin(2 * np.pi * k / lap),
                                                        0.3 * np.sin(6 * np.pi * k / lap)]) for k in range(n)]
    ops = [("prior", 0, gt[0])]
    for k in range(n - 1):
        ops.append(("odom", k, k + 1, rel(gt[k], gt[k + 1]) @ make_transform([0, 0, 0.001], [0, 0, 0])
                    @ noise(0.004, 0.03), 0.0))
    ops += [("loop", i, j, rel(gt[i], gt[j]) @ noise(0.001, 0.01)) for i, j in true_loops]
    ops.append(("loop", false_loop[0], false_loop[1], noise(0.001, 0.01)))
    return ops


def apply(g, ops):
    for op in ops:
        if op[0] == "prior":
            g.add_prior(op[1], op[2])
        elif op[0] == "odom":
            g.add_odometry_factor(op[1], op[2], op[3], op[4])
        else:
            g.add_loop_closure(op[1], op[2], op[3])


def solve(ops, kind=LOSS_NONE, scale=0.0, ordering="COLAMD"):
    g = PoseGraph()
    g.set_loop_loss(kind, scale)
    apply(g, ops)
    assert g.optimize(ordering)
    return g


def max_deviation(a, b):
    return float(np.max(np.linalg.norm(np.stack(a)[:, :3, 3] - np.stack(b)[:, :3, 3], axis=1)))


def main():
    rows = [(LOSS_NONE, 0.0), (LOSS_HUBER, 1.345), (LOSS_CAUCHY, 1.0), (LOSS_GEMAN_MCCLURE, 10.0),
            (LOSS_GEMAN_MCCLURE, 1.0)]
    print("| loop edges | max deviation from the clean optimum [m] | LM steps / trials | stop | weight of the false edge "
          "| least weight of a true edge |")
    print("|---|---|---|---|---|---|")
    for kind, k in rows:
        dev, steps, stop, wf, wt = [], [], [], [], []
        for seed in (1, 2, 3):
            ops = false_closure_ring(seed)
            clean = solve(ops[:-1]).get_all_poses()
            g = solve(ops, kind, k)
            w, _ = g.loop_weights()
            dev.append("%.4g" % max_deviation(g.get_all_poses(), clean))
            steps.append("%d/%d" % (g.stats.iterations, g.stats.inner_trials))
            stop.append(str(g.stats.stop_reason))
            wf.append("%.2g" % w[-1])
            wt.append("%.3g" % w[:-1].min())
        name = LOSS_NAMES[kind] + (", k = %g" % k if kind else "")
        print("| %s | %s | %s | %s | %s | %s |" % (name, " / ".join(dev), ", ".join(steps), ", ".join(stop),
                                                    " / ".join(wf), " / ".join(wt)))


if __name__ == "__main__":
    main()
