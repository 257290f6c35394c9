"""Plane-to-plane loop verification off the device: the L12 drive through scripts/gicp_ref.GicpOracleBackend
-- gicp_icp behind the yaw-guess detector, the 2 m gate and epsilon = 1e-3 -- next to Huber 0.1 m behind the same gate.
It finds the 13 closures of 13 verifications the Huber run finds, with the same (query, match, shift) triples, closer to
truth and in fewer passes, clear of the stopping test and of the gate; the backend's validation and its cache."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import gated_icp_ref as gr  # noqa: E402
import gicp_ref as ref  # noqa: E402
import loop_yaw_ref as yr  # noqa: E402
import robust_icp_ref as rr  # noqa: E402

# the rows each closure's last pass kept, in result order (the issue's record of this run)
L12_KEPT = [4147, 3159, 2755, 2432, 2876, 4045, 3770, 3370, 4255, 3962, 3949, 4378, 4113]


def test_l12_closes_as_huber_does_closer_and_in_fewer_passes(oracle):
    poses, labels, clouds = gr.l12_scans()
    huber = rr.RobustOracleBackend(rr.HUBER, rr.HUBER_SCALE, gr.L12_GATE, oracle)
    gicp = ref.GicpOracleBackend(ref.EPSILON_DEFAULT, gr.L12_GATE, oracle)
    a = gr.run_detector(yr.YawLoopClosureDetector(huber, gr.l12_config()), clouds, labels)
    b = gr.run_detector(yr.YawLoopClosureDetector(gicp, gr.l12_config()), clouds, labels)
    wa, wb = rr.l12_worst(a, poses, labels), rr.l12_worst(b, poses, labels)
    pa, pb = sum(r.num_iterations for r in huber.runs), sum(r.num_iterations for r in gicp.runs)
    stop, gate = gicp.min_margins()
    print("  L12: Huber + gate %d closures of %d verifications, worst %.4f m, %d passes; plane-to-plane + gate %d of %d, "
          "worst %.4f m, %d passes, largest final_error %.4f; margins %.2e, %.2e m^2"
          % (len(a), len(huber.runs), wa, pa, len(b), len(gicp.runs), wb, pb, max(r.final_error for r in gicp.runs), stop, gate))
    assert len(b) == 13 and len(gicp.runs) == 13
    assert [(c.query_frame, c.match_frame, c.sector_shift) for c in b] == [(c.query_frame, c.match_frame, c.sector_shift) for c in a]
    assert wb < wa and pb < pa
    assert stop >= 1e-9 and gate >= 1e-9
    assert [gicp.run_of(c).pairs for c in b] == L12_KEPT
    # a cloud's normals are formed once, whichever side of a verification it is on
    assert len(gicp._normals) <= len(clouds)
    with pytest.raises(KeyError):
        gicp.run_of(a[0])


@pytest.mark.parametrize("epsilon, gate", [(0.0, 2.0), (-1e-3, 2.0), (1.5, 2.0), (float("nan"), 2.0), (1e-3, -1.0),
                                           (1e-3, float("inf"))])
def test_the_backend_validates_its_rule(epsilon, gate):
    with pytest.raises(ValueError):
        ref.GicpOracleBackend(epsilon, gate, orc=object())


def test_the_backend_passes_the_sources_normals(oracle):
    """the cached normals are the ones gicp_icp would estimate: same bits with and without the backend"""
    clouds = gr.l12_scans()[2]
    s, t, start = gr.l12_pair(clouds, 6, 5, oracle)
    backend = ref.GicpOracleBackend(ref.EPSILON_DEFAULT, gr.L12_GATE, oracle)
    got = backend.align(s, t, 30, 1e-6, initial_transform=start)
    want = ref.gicp_icp(s, t, ref.EPSILON_DEFAULT, gr.L12_GATE, 30, 1e-6, 1e-9, start, orc=oracle)
    assert np.array_equal(got.transformation.view(np.uint64), want.transformation.view(np.uint64))
    assert np.array_equal(got.error_history.view(np.uint64), want.error_history.view(np.uint64)) and got.pairs == want.pairs
    assert backend.iterations == [got.num_iterations] and backend.runs == [got]
