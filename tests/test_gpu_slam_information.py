"""Information edges through the node's loop (slam.run_slam(edge_information=sigma)) on the out-and-back
street of tests/test_gpu_loop_store.py and tests/test_gpu_pose_graph_loss.py (60 frames out, 60 back, 32 beams x 900
azimuths): every good registration's edge carries the matrix icpmi_information_from_icp makes of that registration's own
normal matrix, with the host detector and with the detector on the device; the closures do not depend on the option; the
final poses are the restatement's optimum of the recorded factor list."""
import os
import sys

import numpy as np
import pytest

import torch  # noqa: F401  (first: one HIP runtime per process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import pose_graph_info_ref as I  # noqa: E402
from lidar_slam_from_scratch_amd import capi, slam, synth  # noqa: E402

pytestmark = pytest.mark.gpu

SIGMA, FLOOR = 0.02, (1.0, 10.0)
ORDER = list(range(60)) + list(range(59, -1, -1))


@pytest.fixture(scope="module")
def ctx():
    """Fails loudly (no skip, no fallback) when the HIP library or the device is missing."""
    from lidar_slam_from_scratch_amd import build
    build.build_library()
    c = capi.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def frames():
    cache = {f: synth.lidar_frame(f, beams=32, azimuths=900, **synth.DRIVE_200) for f in set(ORDER)}
    return [cache[f] for f in ORDER]


@pytest.fixture(scope="module")
def runs(ctx, frames):
    """The three runs, once: the option off, on with the host detector, on with the detector on the device."""
    return (slam.run_slam(frames, ctx),
            slam.run_slam(frames, ctx, edge_information=SIGMA, information_floor=FLOOR),
            slam.run_slam(frames, ctx, edge_information=SIGMA, information_floor=FLOOR, loop_on_device=True))


def _ate(poses):
    gt0 = np.linalg.inv(synth.lidar_pose(ORDER[0], **synth.DRIVE_200))
    err = [np.linalg.norm((gt0 @ synth.lidar_pose(f, **synth.DRIVE_200))[:3, 3] - P[:3, 3]) for f, P in zip(ORDER, poses)]
    return float(np.sqrt(np.mean(np.square(err))))


def test_closures_do_not_depend_on_the_option(runs):
    base, host, dev = runs
    assert base.closures
    for run in (host, dev):
        assert [(c.query_frame, c.match_frame) for c in run.closures] == [(c.query_frame, c.match_frame) for c in base.closures]
        for a, b in zip(run.closures, base.closures):
            assert np.array_equal(a.transform, b.transform) and a.icp_fitness == b.icp_fitness
        assert [o[0] for o in run.optimizations] == [o[0] for o in base.optimizations]
        assert all(o[1] for o in run.optimizations) and run.optimizations[-1][1]
    assert all(c.information is None for c in base.closures)
    assert [f[0] for f in base.factors if f[0] != "prior"] == [{"odom_info": "odom", "loop_info": "loop"}.get(f[0], f[0])
                                                               for f in host.factors if f[0] != "prior"]
    print("ATE over %d poses: option off %.4f m, information edges %.4f m (host detector), %.4f m (device detector)"
          % (len(ORDER), _ate(base.poses), _ate(host.poses), _ate(dev.poses)))


def test_every_edge_carries_its_own_registrations_matrix(ctx, frames, runs):
    base, host, dev = runs
    odom = [f for f in host.factors if f[0] in ("odom", "odom_info")]
    assert [(f[1], f[2]) for f in odom] == [(k - 1, k) for k in range(1, len(frames))]
    cfg = capi.Context.make_config(max_iterations=50, tolerance=1e-6)
    n_info = 0
    for f, g in zip(odom, [f for f in base.factors if f[0] == "odom"]):
        k = f[2]
        res, _hist = ctx.align(frames[k], frames[k - 1], cfg)        # the same pair, alone
        bad = (not res.converged) or res.final_error > 1.0
        assert (f[0] == "odom") == bad
        assert np.array_equal(f[3], g[3])                            # the transform is the plain run's
        if bad:
            assert np.array_equal(f[3], np.eye(4)) and f[4] == g[4]  # the identity under the diagonal model, as before
            continue
        nm = ctx.last_normal_matrix()
        assert np.array_equal(nm.T, f[3])
        assert np.array_equal(f[4], capi.information_from_icp(nm.JtJ, nm.T, SIGMA, *FLOOR))
        assert np.array_equal(f[4], I.information_from_icp(nm.JtJ, nm.T, SIGMA, *FLOOR))
        I.cholesky_upper(f[4])                                       # positive definite, symmetric
        n_info += 1
    assert n_info > 100
    cfg = capi.Context.make_config(max_iterations=30, tolerance=1e-6)
    loops = [f for f in host.factors if f[0] == "loop_info"]
    assert len(loops) == len(host.closures) > 0 and not [f for f in host.factors if f[0] == "loop"]
    for f, c in zip(loops, host.closures):
        assert (f[1], f[2]) == (c.match_frame, c.query_frame) and f[4] is c.information
        ctx.align(frames[c.query_frame], frames[c.match_frame], cfg)
        nm = ctx.last_normal_matrix()
        assert np.array_equal(nm.T, f[3])
        assert np.array_equal(f[4], capi.information_from_icp(nm.JtJ, nm.T, SIGMA, *FLOOR))


def test_device_detector_hands_over_the_same_matrices(runs):
    """icpmi_loop_last_information against the host detector's, bit for bit -- and with them the whole run."""
    _base, host, dev = runs
    assert len(host.factors) == len(dev.factors)
    for f, g in zip(host.factors, dev.factors):
        assert f[0] == g[0] and len(f) == len(g)
        assert all(np.array_equal(x, y) for x, y in zip(f[1:], g[1:]))
    for a, b in zip(host.closures, dev.closures):
        assert a.information is not None and np.array_equal(a.information, b.information)
    assert np.array_equal(np.stack(host.poses), np.stack(dev.poses))


def test_final_poses_are_the_restatements_optimum(runs):
    _base, host, _dev = runs
    ref = I.PoseGraph()
    I.apply(ref, host.factors)
    assert ref.optimize("COLAMD")
    a, sa = np.stack(ref.get_all_poses()), ref.stats
    assert ref.optimize("NATURAL")
    b = np.stack(ref.get_all_poses())
    assert sa.min_margin > 1e-6
    got = np.stack(host.poses)
    n = len(got)
    tol = np.maximum(10 * np.abs(a - b).reshape(n, -1).max(axis=1), 1e-12 * (1 + np.linalg.norm(a[:, :3, 3], axis=1)))
    assert (np.abs(got - a).reshape(n, -1).max(axis=1) <= tol).all()
    st = host.optimizations[-1][2]
    assert (st.iterations, st.inner_trials) == (sa.iterations, sa.inner_trials)


def test_the_option_composes(ctx, frames):
    """With the gate, the robust rules, the loop-edge loss and scan-to-local-map odometry: the run ends with a
    successful optimize and every good edge is an information edge."""
    from lidar_slam_from_scratch_amd.local_map import LocalMapConfig
    short = frames[:8]
    run = slam.run_slam(short, ctx, edge_information=SIGMA, odom_robust=(capi.ROBUST_HUBER, 0.05), loop_gate=2.0,
                        loop_robust=(capi.ROBUST_HUBER, 0.05), loop_edge_loss=(capi.PG_LOSS_CAUCHY, 1.0))
    assert run.optimizations[-1][1] and [f[0] for f in run.factors[1:]] == ["odom_info"] * 7
    run = slam.run_slam(short, ctx, edge_information=SIGMA, odom_local_map=LocalMapConfig())
    assert run.optimizations[-1][1] and [f[0] for f in run.factors[1:]] == ["odom_info"] * 7
    with pytest.raises(ValueError):
        slam.run_slam(short, ctx, edge_information=SIGMA, align=lambda *a: None)


def test_detectors_agree_under_gate_weights_and_yaw_guess(ctx, frames):
    """The same drive with the verifications gated at 2 m, under Huber weights and started from Scan Context's shift: the
    device detector's matrices (icpmi_loop_last_information) are the host detector's, bit for bit, and each is the one
    of its own verification -- the weighted normal matrix, mapped at that verification's transform."""
    kw = dict(edge_information=SIGMA, information_floor=FLOOR, loop_gate=2.0, loop_robust=(capi.ROBUST_HUBER, 0.05),
              loop_yaw_guess=True)
    host = slam.run_slam(frames, ctx, **kw)
    dev = slam.run_slam(frames, ctx, loop_on_device=True, **kw)
    assert host.closures and len(host.closures) == len(dev.closures)
    for a, b in zip(host.closures, dev.closures):
        assert (a.query_frame, a.match_frame, a.sector_shift) == (b.query_frame, b.match_frame, b.sector_shift)
        assert np.array_equal(a.transform, b.transform) and np.array_equal(a.information, b.information)
        I.cholesky_upper(a.information)
    from lidar_slam_from_scratch_amd import loop_closure as lc
    c = host.closures[0]
    cfg = capi.Context.make_config(max_iterations=30, tolerance=1e-6, initial_transform=lc.sc_shift_transform(c.sector_shift))
    res, _hist, info = ctx.align_robust(frames[c.query_frame], frames[c.match_frame], cfg, (capi.ROBUST_HUBER, 0.05, 2.0))
    nm = ctx.last_normal_matrix()
    assert np.array_equal(nm.T, c.transform) and nm.weight == info.weight_sum == c.weight_sum and nm.pairs == c.pairs
    assert np.array_equal(c.information, capi.information_from_icp(nm.JtJ, nm.T, SIGMA, *FLOOR))
    assert all(o[1] for o in host.optimizations)
