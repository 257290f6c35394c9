#!/usr/bin/env python3
"""Pose-graph back end timing on a KITTI-00-shaped graph: 4,541 poses, 4,540 odometry factors and three closures per
query on later laps (the graph of tests/test_gpu_pose_graph.py::test_kitti_shaped_graph).

    python scripts/pose_graph_timing.py            device: one full optimize() (median of 7), then the node's pattern
                                                   (optimize after every query's closures on the growing graph, and at
                                                   the end), summed; one JSON line
    python scripts/pose_graph_timing.py --once     one optimize() only (to put under rocprofv3 --kernel-trace --stats)
    python scripts/pose_graph_timing.py --ref      the same two measurements with scripts/pose_graph_ref.py (CPU)

Host clock around calls that end synchronised (icpmi_pose_graph_optimize reads its result back)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import pose_graph_ref as R  # noqa: E402
from lidar_slam_from_scratch_amd import synth  # noqa: E402


def kitti_ops(seed=7, n=4541, lap=900, every=30):
    rng = np.random.default_rng(seed)

    def noise(rs, ts):
        return R.se3_exp(np.r_[rng.normal(0, rs, 3), rng.normal(0, ts, 3)])

    gt = []
    for k in range(n):
        a = 2 * np.pi * (k % lap) / lap
        gt.append(synth.make_transform([0, 0, a], [200 * np.cos(a), 120 * np.sin(a), 2 * np.sin(3 * a)]))
    rel = lambda a, b: np.linalg.inv(a) @ b   # noqa: E731
    ops = [("prior", 0, gt[0])]
    ops += [("odom", k, k + 1, rel(gt[k], gt[k + 1]) @ noise(0.002, 0.02), 0.02 * rng.uniform()) for k in range(n - 1)]
    for q in range(lap + 60, n, every):
        for m in (q - lap - 1, q - lap, q - lap + 2):
            ops.append(("loop", m, q, rel(gt[m], gt[q]) @ noise(0.001, 0.01)))
    return ops


def apply(g, ops):
    for op in ops:
        if op[0] == "prior":
            g.add_prior(op[1], op[2])
        elif op[0] == "odom":
            g.add_odometry_factor(op[1], op[2], op[3], op[4])
        else:
            g.add_loop_closure(op[1], op[2], op[3])


def node_pattern(make, ops):
    """Factors in the node's order (odometry up to the query frame, then its closures), optimize after each query's
    closures and once at the end; returns (seconds summed over the optimize calls, number of calls)."""
    loops = {}
    for op in ops:
        if op[0] == "loop":
            loops.setdefault(op[2], []).append(op)
    g = make()
    apply(g, ops[:1])
    total, calls = 0.0, 0
    for op in ops[1:]:
        if op[0] != "odom":
            continue
        apply(g, [op])
        q = op[2]
        if q in loops:
            apply(g, loops[q])
            t0 = time.perf_counter()
            assert g.optimize()
            total += time.perf_counter() - t0
            calls += 1
    t0 = time.perf_counter()
    assert g.optimize()
    return total + time.perf_counter() - t0, calls + 1


def main():
    ops = kitti_ops()
    out = {"poses": 4541, "odometry": sum(o[0] == "odom" for o in ops), "closures": sum(o[0] == "loop" for o in ops)}
    if "--ref" in sys.argv:
        make = R.PoseGraph
        out["side"] = "restatement (numpy + splu COLAMD, CPU)"
    else:
        import torch  # noqa: F401
        from lidar_slam_from_scratch_amd import capi, pose_graph
        ctx = capi.Context(device=0)
        make = lambda: pose_graph.PoseGraph(ctx)   # noqa: E731
        out["side"] = "device"
    g = make()
    apply(g, ops)
    reps = 1 if "--once" in sys.argv else 7
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        assert g.optimize()
        ts.append(time.perf_counter() - t0)
    st = g.stats
    out.update(full_optimize_ms_median=1e3 * float(np.median(ts)), full_optimize_ms_all=[round(1e3 * t, 3) for t in ts],
               iterations=st.iterations, inner_trials=st.inner_trials, final_error=st.final_error)
    if "--once" not in sys.argv:
        tot, calls = node_pattern(make, ops)
        out.update(node_pattern_ms_total=1e3 * tot, node_pattern_calls=calls)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
