"""The CPU restatement of ICP behind a correspondence-distance gate (scripts/gated_icp_ref.py): with a gate
that keeps every row it is the oracle's icp_point_to_plane; on L12 -- R12 with the return leg 1.5 m aside -- a 2 m gate
closes every return scan where the ungated detector leaves some without a closure; the kept sets of every fixture the
GPU tests compare by `pairs` are far from hanging on rounding; the no-pairs rule; the history invariants on
all three ways out of the loop."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import gated_icp_ref as ref  # noqa: E402
import loop_yaw_ref as yr  # noqa: E402
from lidar_slam_from_scratch_amd import synth  # noqa: E402


@pytest.fixture(scope="module")
def l12():
    return ref.l12_scans()


@pytest.fixture(scope="module")
def l12_gated(oracle, l12):
    """-> (backend, closures) of the gated detector over L12, once"""
    _, labels, clouds = l12
    backend = ref.GatedOracleBackend(ref.L12_GATE, oracle)
    return backend, ref.run_detector(yr.YawLoopClosureDetector(backend, ref.l12_config()), clouds, labels)


def _same_as_oracle(oracle, src, tgt, max_iterations, start=None):
    want = oracle.icp_point_to_plane(src, tgt, max_iterations, 1e-6, 1e-9, initial_transform=start)
    got = ref.gated_icp(src, tgt, 1e6, max_iterations, 1e-6, 1e-9, start, orc=oracle)
    assert np.abs(got.transformation - want.transformation).max() <= 1e-12
    assert got.num_iterations == want.num_iterations and got.converged == want.converged
    assert got.pairs == src.shape[0]
    assert np.abs(got.error_history - want.error_history).max() <= 1e-12


def test_a_gate_that_keeps_all_is_the_oracle(oracle, l12):
    src, tgt, _ = synth.c1_room_corner(1001)
    _same_as_oracle(oracle, src, tgt, 50)
    s, t, start = ref.l12_pair(l12[2], 6, 5, oracle)
    _same_as_oracle(oracle, s, t, 30, start)


def test_l12_closes_with_the_gate_and_not_without(oracle, l12, l12_gated):
    poses, labels, clouds = l12
    backend, gated = l12_gated
    assert {c.query_frame for c in gated} == set(range(100, 106))
    for c in gated:
        dt, dr = synth.pose_delta(c.transform, yr.truth(poses, labels.index(c.query_frame), labels.index(c.match_frame)))
        print("  gated (%d, %d): %.3f m %.3f deg, pairs %d" % (c.query_frame, c.match_frame, dt, math.degrees(dr), backend.run_of(c).pairs))
        assert dt <= 0.25 and math.degrees(dr) <= 0.5
    ungated = ref.run_detector(yr.YawLoopClosureDetector(yr.OracleBackend(oracle), ref.l12_config()), clouds, labels)
    assert set(range(100, 106)) - {c.query_frame for c in ungated}


def test_kept_sets_do_not_hang_on_rounding(oracle, l12, l12_gated):
    """a condition on the fixtures tests/test_gpu_gated.py compares by `pairs`: the closest any row of any pass comes
    to the gate, |d2 - g2|, is far above what the device's and the oracle's roundings of a pose can differ by"""
    margins = {"L12 detector": l12_gated[0].min_margin()}
    for q, m in ref.L12_PAIRS:
        s, t, start = ref.l12_pair(l12[2], q, m, oracle)
        margins["L12 pair (%d, %d)" % (q, m)] = ref.gated_icp(s, t, ref.L12_GATE, 30, 1e-6, 1e-9, start, orc=oracle).min_margin
    s, t = ref.general_pair()
    margins["general pair"] = ref.gated_icp(s, t, ref.L12_GATE, 30, 1e-6, 1e-9, orc=oracle).min_margin
    print(margins)
    assert min(margins.values()) > 1e-9


def _history_invariants(r, max_iterations):
    """num_iterations = len(history) - 1; at most max_iterations + 1 entries; final_error is the last"""
    h = r.error_history
    assert r.num_iterations == len(h) - 1 and 1 <= len(h) <= max_iterations + 1
    assert r.final_error == h[-1] or (math.isnan(r.final_error) and math.isnan(h[-1]))


def test_no_pairs_ends_the_call_like_a_break(oracle):
    src, tgt, _ = synth.c1_room_corner(1001)
    r = ref.gated_icp(src + np.array([100.0, 0.0, 0.0]), tgt, 1.0, 50, 1e-6, 1e-9, orc=oracle)
    assert r.error_history.tolist() == [math.inf, math.inf] and r.final_error == math.inf
    assert not r.converged and r.pairs == 0 and r.num_iterations == 1
    assert np.array_equal(r.transformation, np.eye(4))
    _history_invariants(r, 50)


def test_history_invariants_on_the_three_ways_out(oracle, l12):
    s, t, start = ref.l12_pair(l12[2], 8, 3, oracle)
    broke = ref.gated_icp(s, t, ref.L12_GATE, 30, 1e-6, 1e-9, start, orc=oracle)          # a convergence break
    assert broke.converged and broke.num_iterations < 30 and broke.error_history[-1] == broke.error_history[-2]
    _history_invariants(broke, 30)
    spent = ref.gated_icp(s, t, ref.L12_GATE, 3, 1e-6, 1e-9, start, orc=oracle)           # exhausted
    assert not spent.converged and len(spent.error_history) == 4
    _history_invariants(spent, 3)
    assert np.array_equal(spent.error_history[:3], broke.error_history[:3])
    # no pairs: the source lifted 50 m above the street, a 1 m gate
    none = ref.gated_icp(s + np.array([0.0, 0.0, 50.0]), t, 1.0, 30, 1e-6, 1e-9, start, orc=oracle)
    assert not none.converged and none.error_history.tolist() == [math.inf, math.inf]
    _history_invariants(none, 30)
    with pytest.raises(ValueError):
        ref.gated_icp(s, t, 0.0, orc=oracle)
    with pytest.raises(ValueError):
        ref.gated_icp(s, t, math.inf, orc=oracle)
