"""The CPU restatement of the robust loss on loop-closure edges (scripts/pose_graph_loss_ref.py) on the graph it is for:
a two-lap ring of 200 poses, 30 m radius, 9 true closures and one false closure between poses 30 and 150 (57 m apart,
measurement about identity).  Deviations are the largest translation distance of any pose from the plain optimum of the
same draw without the false closure.  Thresholds are the issue's (measured: plain 32.4-32.7 m, Huber 1.53-1.54 m,
Cauchy <= 0.0012 m, Geman-McClure(10) < 5e-5 m).  Runs on the CPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import pose_graph_loss_ref as L  # noqa: E402
import pose_graph_ref as R  # noqa: E402
from lidar_slam_from_scratch_amd import synth  # noqa: E402
from test_gpu_pose_graph import _noise, _rel, apply, chain_ops  # noqa: E402

SEEDS = [1, 2, 3]


def ring_false_ops(seed, lap=100):
    """The issue's generator, in the helpers' terms of tests/test_gpu_pose_graph.py; ops[:-1] is the clean graph."""
    n = 2 * lap
    rng = np.random.default_rng(seed)
    gt = [synth.make_transform([0, 0, 2 * np.pi * k / lap], [30 * np.cos(2 * np.pi * k / lap),
                                                             30 * np.sin(2 * np.pi * k / lap),
                                                             0.3 * np.sin(6 * np.pi * k / lap)]) for k in range(n)]
    ops = [("prior", 0, gt[0])]
    for k in range(n - 1):
        ops.append(("odom", k, k + 1, _rel(gt[k], gt[k + 1]) @ synth.make_transform([0, 0, 0.001], [0, 0, 0])
                    @ _noise(rng, 0.004, 0.03), 0.0))
    ops += [("loop", k, k + lap, _rel(gt[k], gt[k + lap]) @ _noise(rng, 0.001, 0.01)) for k in range(10, lap, 10)]
    ops.append(("loop", 30, 150, _noise(rng, 0.001, 0.01)))
    return ops


_cache = {}


def solved(seed, kind=L.LOSS_NONE, scale=0.0, clean=False):
    """One optimum per (seed, loss), shared by the tests and left unchanged."""
    key = (seed, kind, scale, clean)
    if key not in _cache:
        ops = ring_false_ops(seed)
        _cache[key] = L.solve(ops[:-1] if clean else ops, kind, scale)
    return _cache[key]


def deviation(seed, kind=L.LOSS_NONE, scale=0.0):
    return L.max_deviation(solved(seed, kind, scale).get_all_poses(), solved(seed, clean=True).get_all_poses())


def test_generators_agree():
    """The program's table (pose_graph_loss_ref.false_closure_ring) is of the same graph as these tests."""
    for a, b in zip(ring_false_ops(1), L.false_closure_ring(1, make_transform=synth.make_transform)):
        assert a[:2] == b[:2] and all(np.array_equal(x, y) for x, y in zip(a[2:], b[2:]))


@pytest.mark.parametrize("seed", SEEDS)
def test_one_false_closure_bends_the_plain_optimum(seed):
    d = deviation(seed)
    print("plain deviation", seed, d, solved(seed).stats.iterations, solved(seed).stats.inner_trials)
    assert d > 10.0


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kind,scale", [(L.LOSS_CAUCHY, 1.0), (L.LOSS_GEMAN_MCCLURE, 10.0)])
def test_redescending_loss_gives_the_clean_optimum_back(seed, kind, scale):
    d = deviation(seed, kind, scale)
    print("deviation", L.LOSS_NAMES[kind], scale, seed, d)
    assert d < 0.05


@pytest.mark.parametrize("seed", SEEDS)
def test_huber_lies_between(seed):
    h = deviation(seed, L.LOSS_HUBER, 1.345)
    print("huber deviation", seed, h)
    assert max(deviation(seed, L.LOSS_CAUCHY, 1.0), deviation(seed, L.LOSS_GEMAN_MCCLURE, 10.0)) < h < deviation(seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_cauchy_weights_name_the_false_edge(seed):
    w, d = solved(seed, L.LOSS_CAUCHY, 1.0).loop_weights()
    print("cauchy weights", seed, w, d)
    assert len(w) == 10
    assert w[-1] < 1e-3
    assert (w[:-1] > 0.5).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_hazard_scale_below_the_drift_rejects_every_closure(seed):
    """Documented behaviour, not a wish: optimize() starts from the drifted estimates, where every true closure is tens
    of sigmas out; Geman-McClure of scale 1 switches them all off and stops after one step."""
    g = solved(seed, L.LOSS_GEMAN_MCCLURE, 1.0)
    w, _ = g.loop_weights()
    print("hazard weights", seed, w, g.stats.iterations)
    assert (w < 1e-3).all()


@pytest.mark.parametrize("kind", [L.LOSS_HUBER, L.LOSS_CAUCHY, L.LOSS_GEMAN_MCCLURE])
@pytest.mark.parametrize("k", [0.5, 1.345, 10.0])
def test_weight_is_the_derivative_of_rho_over_d(kind, k):
    """w = rho'(d) / d by a central difference, d from 1e-6 to 1e4, compared as rho'(d) = w d.  With h = 1e-4 d the
    quotient's truncation error is h^2 rho''' / 6, for these losses a small multiple of (h / d)^2 = 1e-8 of w d (Huber:
    zero away from d = k, whose neighbourhood is left out); the bound allows 1e-6 w d.  rho itself is rounded to a few
    eps, which the quotient magnifies to eps rho / h; the bound allows 4 eps rho / h for it."""
    d = np.logspace(-6, 4, 201)
    if kind == L.LOSS_HUBER:
        d = d[np.abs(d - k) > 1e-3 * k]
    h = 1e-4 * d
    w, rho, sw = L.loss_weight_rho(d, kind, k)
    up, dn = L.loss_weight_rho(d + h, kind, k)[1], L.loss_weight_rho(d - h, kind, k)[1]
    slope = (up - dn) / (2 * h)
    tol = 1e-6 * w * d + 4 * np.finfo(np.float64).eps * rho / h
    assert (np.abs(slope - w * d) <= tol).all(), float(np.max(np.abs(slope - w * d) / tol))
    assert np.allclose(sw * sw, w, rtol=1e-15, atol=0)
    assert (w > 0).all() and (w <= 1).all() and np.isfinite(rho).all()


@pytest.mark.parametrize("k", [0.5, 1.345, 10.0])
def test_huber_is_continuous_at_its_knee(k):
    e = 1e-9 * k
    (w0, r0, _), (w1, r1, _), (wk, rk, _) = (L.loss_weight_rho(x, L.LOSS_HUBER, k) for x in (k - e, k + e, k))
    assert wk == 1.0 and rk == 0.5 * k * k
    assert abs(w1 - w0) <= 2e-9 and abs(r1 - r0) <= 4e-9 * k * k


def test_zero_distance_is_finite():
    for kind in (L.LOSS_HUBER, L.LOSS_CAUCHY, L.LOSS_GEMAN_MCCLURE):
        w, rho, sw = L.loss_weight_rho(np.zeros(3), kind, 1.0)
        assert (w == 1.0).all() and (rho == 0.0).all() and (sw == 1.0).all()


def _lm(ops, **hooks):
    g = R.PoseGraph()
    apply(g, ops)
    keys, kind, fi, fj, Z, inv_sigma, X0 = g.arrays()
    return (kind, fi, fj, Z, inv_sigma, X0), R.levenberg_marquardt(kind, fi, fj, Z, inv_sigma, X0, g.config, **hooks)


def test_default_hooks_change_nothing():
    """levenberg_marquardt with its hooks left alone, on chain_ops(20, 9): bit for bit what passing the present
    functions gives, its initial and final errors bit for bit total_error's, and its poses, history, counts and lambda
    those recorded from the code before the hooks existed (tests/golden/pose_graph_lm_chain20.npz; compared to
    1e-12 (1 + |t|) and not bitwise, since the stored numbers went through another machine's BLAS)."""
    arrays, (X, st) = _lm(chain_ops(20, 9))
    _, (X2, st2) = _lm(chain_ops(20, 9), linearize=R._linearize, errors=R.factor_errors)
    assert (X == X2).all() and st.history == st2.history and st.final_lambda == st2.final_lambda
    assert (st.iterations, st.inner_trials, st.stop_reason) == (st2.iterations, st2.inner_trials, st2.stop_reason)
    kind, fi, fj, Z, inv_sigma, X0 = arrays
    assert st.history[0] == R.total_error(kind, fi, fj, Z, inv_sigma, X0)
    assert st.final_error == R.total_error(kind, fi, fj, Z, inv_sigma, X)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "pose_graph_lm_chain20.npz"))
    assert [st.iterations, st.inner_trials, st.stop_reason] == gold["counts"].tolist()
    assert st.final_lambda == float(gold["final_lambda"])
    tol = 1e-12 * (1.0 + np.linalg.norm(gold["poses"][:, :3, 3], axis=1))
    assert (np.abs(X - gold["poses"]).reshape(len(X), -1).max(axis=1) <= tol).all()
    assert np.allclose(st.history, gold["history"], rtol=1e-12, atol=0)


def test_loss_restatement_with_the_loss_off_is_the_plain_one():
    """The subclass with kind 0, or with a loss and no loop factor, runs the plain hooks: bit-equal to pose_graph_ref."""
    ops = ring_false_ops(1)
    plain = R.PoseGraph()
    apply(plain, ops)
    assert plain.optimize()
    assert (np.stack(solved(1).get_all_poses()) == np.stack(plain.get_all_poses())).all()
    assert solved(1).stats.history == plain.stats.history
    chain = chain_ops(20, 9)
    a = L.solve(chain, L.LOSS_CAUCHY, 1.0)
    b = R.PoseGraph()
    apply(b, chain)
    assert b.optimize()
    assert (np.stack(a.get_all_poses()) == np.stack(b.get_all_poses())).all() and a.stats.history == b.stats.history


def test_setting_rules():
    g = L.PoseGraph()
    for bad in ((4, 1.0), (-1, 1.0), (1, 0.0), (2, -1.0), (3, float("nan")), (1, float("inf"))):
        with pytest.raises(R.PoseGraphError):
            g.set_loop_loss(*bad)
        assert g.loop_loss() == (L.LOSS_NONE, 0.0)
    apply(g, chain_ops(5, 1))
    assert g.optimize()
    g.set_loop_loss(L.LOSS_NONE, 7.0)                 # NONE ignores the scale: a repeat
    assert g.optimized
    g.set_loop_loss(L.LOSS_CAUCHY, 1.0)
    assert not g.optimized and g.loop_loss() == (L.LOSS_CAUCHY, 1.0)
    with pytest.raises(R.PoseGraphError):
        g.loop_weights()
    assert g.optimize()
    g.set_loop_loss(L.LOSS_CAUCHY, 1.0)
    assert g.optimized
    w, d = g.loop_weights()
    assert len(w) == 0 and len(d) == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_huber_margin_is_tracked(seed):
    """min_margin takes |d - k| / k of every Huber loop factor at every linearisation and error evaluation."""
    g = solved(seed, L.LOSS_HUBER, 1.345)
    _, d = g.loop_weights()
    print("huber branch margin", seed, g.stats.min_margin)
    assert g.stats.min_margin <= float(np.min(np.abs(d - 1.345) / 1.345)) * (1 + 1e-9)
    assert g.stats.min_margin > 1e-6
