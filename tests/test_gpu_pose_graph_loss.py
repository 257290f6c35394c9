"""The robust loss on the pose graph's loop-closure edges on the device (icpmi_pose_graph_set_loop_loss / _loop_weights,
csrc/pose_graph_loss.h) against its CPU restatement (scripts/pose_graph_loss_ref.py) on the same factors.

The comparison rule is run_case's of tests/test_gpu_pose_graph.py: poses within 10x the restatement's own COLAMD /
NATURAL spread, at least 1e-12 (1 + |t|); the same for the error history; iterations, trials and stop reason equal.  A
case whose nearest decision (the LM tests, and |d - k| / k of every Huber loop factor) has a relative margin <= 1e-6 in
the restatement gets another seed, never an excuse.

loop_weights() is compared with loss_weight_rho of the restatement's residuals evaluated at the device's own optimised
poses, to 1e-9 (1 + w) and 1e-9 (1 + d): identical doubles go in, so only operation order differs, a few ulp of a 30 m
translation difference (1e-14 m), at most 1e-11 in d after whitening by 1 / 0.005, and |dw/dd| <= 1 / k."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import pose_graph_loss_ref as L  # noqa: E402
import pose_graph_ref as R  # noqa: E402
from lidar_slam_from_scratch_amd import synth  # noqa: E402
from test_gpu_pose_graph import K, _drive, _rel, apply, chain_ops, ring_ops, separators  # noqa: E402
from test_pose_graph_loss_reference import ring_false_ops  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = [(L.LOSS_HUBER, 1.345), (L.LOSS_CAUCHY, 1.0), (L.LOSS_GEMAN_MCCLURE, 10.0)]
IDS = ["huber", "cauchy", "geman_mcclure"]


@pytest.fixture(scope="module")
def ctx():
    """Fails loudly (no skip, no fallback) when the HIP library or the device is missing."""
    from lidar_slam_from_scratch_amd import build, capi
    build.build_library()
    c = capi.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ring():
    """The 200-pose ring with one false closure, seed 1 (ops[:-1]: the clean graph).  Its chain separators 63, 127 and
    191 lie between loop endpoints on either side."""
    ops = ring_false_ops(1)
    assert {63, 127, 191} < separators(ops) and {60, 70, 120, 130, 190} < separators(ops)
    return ops


def small_ring_ops():
    """Nine poses on a ring of radius 5: one true closure (0, 8), one false closure (2, 6); no segment longer than the
    chain between separators."""
    return L.false_closure_ring(5, lap=9, n=9, radius=5.0, true_loops=[(0, 8)], false_loop=(2, 6),
                                make_transform=synth.make_transform)


def device_graph(ctx, ops, kind=None, scale=0.0, max_iterations=100):
    from lidar_slam_from_scratch_amd import pose_graph as pg
    dev = pg.PoseGraph(ctx, pg.PoseGraphConfig(max_iterations=max_iterations))
    if kind is not None:
        dev.set_loop_loss(kind, scale)
    apply(dev, ops)
    return dev


def run_loss_case(ctx, ops, kind, scale):
    """run_case of tests/test_gpu_pose_graph.py with the loss set on both sides.  -> (device graph, its stats,
    the restatement's graph)"""
    ref = L.PoseGraph(R.PoseGraphConfig())
    ref.set_loop_loss(kind, scale)
    apply(ref, ops)
    assert ref.optimize("COLAMD")
    a, sa = np.stack(ref.get_all_poses()), ref.stats
    assert ref.optimize("NATURAL")
    b, sb = np.stack(ref.get_all_poses()), ref.stats
    assert (sa.iterations, sa.inner_trials) == (sb.iterations, sb.inner_trials)
    assert sa.min_margin > 1e-6, "sensitive case: change its seed (margin %.3g)" % sa.min_margin
    dev = device_graph(ctx, ops, kind, scale)
    assert dev.loop_loss() == (kind, scale)
    assert dev.optimize()
    got = np.stack(dev.get_all_poses())
    st = dev.stats
    assert got.shape == a.shape
    print("steps/trials/stop", (st.iterations, st.inner_trials, st.stop_reason), "restatement",
          (sa.iterations, sa.inner_trials, sa.stop_reason), "margin", sa.min_margin)
    assert (st.iterations, st.inner_trials, st.stop_reason) == (sa.iterations, sa.inner_trials, sa.stop_reason)
    spread = np.abs(a - b).reshape(len(a), -1).max(axis=1)
    hs = np.abs(np.array(sa.history) - np.array(sb.history))
    floor = 1e-12 * (1.0 + np.linalg.norm(a[:, :3, 3], axis=1))
    tol = np.maximum(10 * spread, floor)
    err = np.abs(got - a).reshape(len(a), -1).max(axis=1)
    print("pose error / tolerance", float(np.max(err / tol)), "spread", float(spread.max()), "error", float(err.max()))
    assert (err <= tol).all(), (int(np.argmax(err / tol)), float(np.max(err / tol)))
    htol = np.maximum(10 * hs, 1e-12 * (1 + np.abs(sa.history)))
    assert len(st.history) == len(sa.history)
    assert (np.abs(np.array(st.history) - sa.history) <= htol).all(), (st.history, sa.history)
    assert st.final_error == st.history[-1] and st.initial_error == st.history[0]
    return dev, st, ref


def check_weights(weights, distances, poses, ref, kind, scale):
    """The device's (w, d) against the restatement's residuals at the device's own poses."""
    dref = ref.loop_distances_at(poses)
    wref = L.loss_weight_rho(dref, kind, scale)[0]
    assert weights.shape == wref.shape and distances.shape == dref.shape
    ew, ed = np.abs(weights - wref), np.abs(distances - dref)
    print("weights", weights, "distances", distances, "max |dw|", float(ew.max()), "max |dd|", float(ed.max()))
    assert (ew <= 1e-9 * (1 + wref)).all() and (ed <= 1e-9 * (1 + dref)).all()
    return wref, dref


@pytest.mark.parametrize("kind,scale", KINDS, ids=IDS)
def test_ring_with_a_false_closure(ctx, ring, kind, scale):
    dev, st, ref = run_loss_case(ctx, ring, kind, scale)
    w, d = dev.loop_weights()
    check_weights(w, d, dev.get_all_poses(), ref, kind, scale)
    assert len(w) == 10 and int(np.argmin(w)) == 9 and w[9] < 1e-2


@pytest.mark.parametrize("kind,scale", KINDS, ids=IDS)
def test_nine_pose_ring(ctx, kind, scale):
    ops = small_ring_ops()
    assert separators(ops) == {0, 8, 2, 6}
    dev, st, ref = run_loss_case(ctx, ops, kind, scale)
    w, d = dev.loop_weights()
    check_weights(w, d, dev.get_all_poses(), ref, kind, scale)
    assert int(np.argmin(w)) == 1


def test_every_closure_rejected(ctx, ring):
    """Geman-McClure of scale 1, below the drift in sigmas: every loop block is about zero and the reduced system, whose
    separators stay, must still factor (the chain, the prior and lambda keep it positive definite)."""
    dev, st, ref = run_loss_case(ctx, ring, L.LOSS_GEMAN_MCCLURE, 1.0)
    w, d = dev.loop_weights()
    check_weights(w, d, dev.get_all_poses(), ref, L.LOSS_GEMAN_MCCLURE, 1.0)
    assert (w < 1e-3).all() and st.iterations >= 1


def _state(dev):
    st = dev.stats
    return (np.stack(dev.get_all_poses()), st.history, (st.optimized, st.iterations, st.inner_trials, st.stop_reason,
                                                        st.initial_error, st.final_error, st.final_lambda))


def _same(a, b):
    return (a[0] == b[0]).all() and a[1] == b[1] and a[2] == b[2]


def test_loss_without_a_loop_factor_is_the_plain_graph(ctx):
    ops = chain_ops(K + 1, seed=K + 1)
    plain = device_graph(ctx, ops)
    assert plain.optimize()
    loss = device_graph(ctx, ops, L.LOSS_CAUCHY, 1.0)
    assert loss.optimize()
    assert _same(_state(plain), _state(loss))
    w, d = loss.loop_weights()
    assert len(w) == 0 and len(d) == 0


def test_loss_set_and_taken_back_is_the_plain_graph(ctx, ring):
    plain = device_graph(ctx, ring)
    assert plain.optimize()
    back = device_graph(ctx, ring, L.LOSS_GEMAN_MCCLURE, 10.0)
    back.set_loop_loss(L.LOSS_NONE, 3.0)
    assert back.loop_loss() == (L.LOSS_NONE, 0.0)
    assert back.optimize()
    assert _same(_state(plain), _state(back))
    # with the loss off: weights of 1 and the real distances
    w, d = back.loop_weights()
    ref = L.PoseGraph()
    apply(ref, ring)
    check_weights(w, d, back.get_all_poses(), ref, L.LOSS_NONE, 0.0)
    assert (w == 1.0).all() and int(np.argmax(d)) == 9 and d[9] > 10.0     # the bent optimum shares the false edge out


@pytest.mark.parametrize("kind,scale", KINDS, ids=IDS)
def test_exact_closure_has_distance_zero(ctx, kind, scale):
    """A noise-free chain and an exact closure: d is rounding only.  Everything stays finite, Huber's weight is exactly
    1 and the others are within 1e-12 of it (w >= 1 - d^2 / k^2 with d ~ 1e-10)."""
    n = 40
    gt = _drive(n, 11)
    ops = [("prior", 0, gt[0])] + [("odom", k, k + 1, _rel(gt[k], gt[k + 1]), 0.0) for k in range(n - 1)]
    ops.append(("loop", 3, n - 2, _rel(gt[3], gt[n - 2])))
    dev = device_graph(ctx, ops, kind, scale)
    assert dev.optimize()
    st = dev.stats
    assert np.isfinite(np.stack(dev.get_all_poses())).all() and np.isfinite(st.history).all()
    assert np.isfinite([st.initial_error, st.final_error, st.final_lambda]).all()
    w, d = dev.loop_weights()
    print("exact closure", st.iterations, st.inner_trials, st.stop_reason, st.history, w, d)
    assert np.isfinite(d).all() and d[0] < 1e-6
    if kind == L.LOSS_HUBER:
        assert w[0] == 1.0
    else:
        assert abs(w[0] - 1.0) <= 1e-12


def test_a_false_closure_on_the_device(ctx, ring):
    """The CPU tests' functional assertion, on the device and with their thresholds: one false closure costs the plain
    optimum more than 10 m; under Cauchy(1) it is within 0.05 m of the clean optimum, and the false edge is the one
    loop_weights() names."""
    clean = device_graph(ctx, ring[:-1])
    plain = device_graph(ctx, ring)
    cauchy = device_graph(ctx, ring, L.LOSS_CAUCHY, 1.0)
    assert clean.optimize() and plain.optimize() and cauchy.optimize()
    base = clean.get_all_poses()
    dp, dc = L.max_deviation(plain.get_all_poses(), base), L.max_deviation(cauchy.get_all_poses(), base)
    w, _ = cauchy.loop_weights()
    print("deviation: plain", dp, "cauchy", dc, "weights", w)
    assert dp > 10.0
    assert dc < 0.05
    assert int(np.argmin(w)) == 9 and w[9] < 1e-3 and (w[:9] > 0.5).all()


def test_repeated_optimize_under_a_loss_is_bit_identical(ctx, ring):
    dev = device_graph(ctx, ring, L.LOSS_CAUCHY, 1.0)
    assert dev.optimize()
    a = _state(dev)
    w1, d1 = dev.loop_weights()
    w2, d2 = dev.loop_weights()
    assert (w1 == w2).all() and (d1 == d2).all()
    assert dev.optimize()
    assert _same(a, _state(dev))
    w3, d3 = dev.loop_weights()
    assert (w1 == w3).all() and (d1 == d3).all()


def test_error_paths(ctx):
    from lidar_slam_from_scratch_amd import capi
    dev = device_graph(ctx, ring_ops(20, 2, [(0, 15), (3, 18)]))

    def refused(call, code=capi.ERR_ARG):
        with pytest.raises(capi.IcpError) as e:
            call()
        assert e.value.code == code

    refused(dev.loop_weights)                                         # before any optimize
    assert dev.optimize()
    w0, d0 = dev.loop_weights()
    assert (w0 == 1.0).all() and len(d0) == 2
    for kind, scale in ((4, 1.0), (-1, 1.0), (capi.PG_LOSS_HUBER, 0.0), (capi.PG_LOSS_CAUCHY, -1.0),
                        (capi.PG_LOSS_GEMAN_MCCLURE, float("nan")), (capi.PG_LOSS_HUBER, float("inf")),
                        (capi.PG_LOSS_CAUCHY, float("-inf"))):
        refused(lambda: dev.set_loop_loss(kind, scale))
        assert dev.loop_loss() == (capi.PG_LOSS_NONE, 0.0)            # nothing changed:
        w, d = dev.loop_weights()                                     # ... the optimised state holds too
        assert (w == w0).all() and (d == d0).all()
    opt3 = dev.get_pose(3)
    dev.set_loop_loss(capi.PG_LOSS_NONE, float("nan"))                # NONE ignores the scale; a repeat changes nothing
    assert (dev.get_pose(3) == opt3).all() and len(dev.loop_weights()[0]) == 2
    # too little room: the count still comes back, and the state is unharmed
    lib, n, buf = capi.load_library(), C.c_int64(0), np.zeros(2)
    assert lib.icpmi_pose_graph_loop_weights(dev._h, capi._dp(buf), None, 1, C.byref(n)) == capi.ERR_CAPACITY
    assert n.value == 2 and (buf == 0.0).all()
    assert lib.icpmi_pose_graph_loop_weights(dev._h, None, capi._dp(buf), 2, C.byref(n)) == capi.OK
    assert (buf == d0).all()
    # a changing set_loop_loss clears the optimised state, as adding a factor does
    dev.set_loop_loss(capi.PG_LOSS_CAUCHY, 2.0)
    assert dev.loop_loss() == (capi.PG_LOSS_CAUCHY, 2.0)
    refused(dev.loop_weights)
    assert not (dev.get_pose(3) == opt3).all()                        # the initial estimate again
    assert dev.optimize()
    dev.set_loop_loss(capi.PG_LOSS_CAUCHY, 2.0)                       # a repeat
    w, d = dev.loop_weights()
    assert len(w) == 2 and (w < 1.0).all()
    dev.add_loop_closure(1, 16, np.eye(4))
    refused(dev.loop_weights)                                         # after an add
    assert dev.loop_loss() == (capi.PG_LOSS_CAUCHY, 2.0)              # the setting outlives it and covers the new edge
    assert dev.optimize()
    assert len(dev.loop_weights()[0]) == 3


@pytest.fixture(scope="module")
def drive_frames():
    order = list(range(60)) + list(range(59, -1, -1))
    cache = {f: synth.lidar_frame(f, beams=32, azimuths=900, **synth.DRIVE_200) for f in set(order)}
    return [cache[f] for f in order]


def _same_factors(a, b):
    return len(a) == len(b) and all(x[:2] == y[:2] and all(np.array_equal(p, q) for p, q in zip(x[2:], y[2:]))
                                    for x, y in zip(a, b))


def test_run_slam_with_a_loop_edge_loss(ctx, drive_frames):
    """The node's loop on the out-and-back drive of test_run_slam_out_and_back under Cauchy(1) on the loop edges: the
    factor list is the plain run's, the final poses are the loss restatement's optimum of it, and the run hands the
    closures' weights over."""
    from lidar_slam_from_scratch_amd import capi, slam
    plain = slam.run_slam(drive_frames, ctx)
    run = slam.run_slam(drive_frames, ctx, loop_edge_loss=(capi.PG_LOSS_CAUCHY, 1.0))
    assert plain.loop_weights is None and plain.loop_distances is None
    assert run.closures and _same_factors(run.factors, plain.factors)
    assert all(o[1] for o in run.optimizations)
    ref = L.PoseGraph()
    ref.set_loop_loss(L.LOSS_CAUCHY, 1.0)
    apply(ref, run.factors)
    assert ref.optimize("COLAMD")
    a, sa = np.stack(ref.get_all_poses()), ref.stats
    assert ref.optimize("NATURAL")
    b = np.stack(ref.get_all_poses())
    assert sa.min_margin > 1e-6
    got = np.stack(run.poses)
    n = len(got)
    tol = np.maximum(10 * np.abs(a - b).reshape(n, -1).max(axis=1), 1e-12 * (1 + np.linalg.norm(a[:, :3, 3], axis=1)))
    assert (np.abs(got - a).reshape(n, -1).max(axis=1) <= tol).all()
    st = run.optimizations[-1][2]
    assert (st.iterations, st.inner_trials) == (sa.iterations, sa.inner_trials)
    assert len(run.loop_weights) == len(run.closures) == len(run.loop_distances)
    check_weights(run.loop_weights, run.loop_distances, run.poses, ref, L.LOSS_CAUCHY, 1.0)
    print("run_slam under a loss: closures", len(run.closures), "steps", st.iterations, "weights", run.loop_weights)


def test_run_slam_sets_the_loss_on_a_graph_of_the_callers(ctx):
    """loop_edge_loss reaches whichever graph is in use, before the prior: the restatement class works there too."""
    from lidar_slam_from_scratch_amd import capi, slam
    ref = L.PoseGraph()
    seen = []
    add_prior = ref.add_prior
    ref.add_prior = lambda *a: (seen.append(ref.loop_loss()), add_prior(*a))
    frames = [synth.lidar_frame(f, beams=16, azimuths=300, **synth.DRIVE_200) for f in range(3)]
    run = slam.run_slam(frames, ctx, pose_graph=ref, min_points=100, loop_edge_loss=(capi.PG_LOSS_HUBER, 1.345))
    assert seen == [(L.LOSS_HUBER, 1.345)]
    assert run.optimizations[-1][1] and len(run.loop_weights) == 0 and len(run.loop_distances) == 0
