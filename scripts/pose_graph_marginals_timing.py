#!/usr/bin/env python3
"""Timing of the pose graph's covariances (icpmi_pose_graph_marginals) on the KITTI-00-shaped graph of
scripts/pose_graph_timing.py: 4,541 poses, 4,540 odometry factors, three closures per query on later laps.

    python scripts/pose_graph_marginals_timing.py            optimize() for scale, then a fresh call (the first after an
                                                             optimize(): it factors H at lam = 0) and a cached call (the
                                                             column solve alone) for q = 1, 4 and 40; medians of 7 after
                                                             a warm-up; one JSON line, also written to
                                                             profiles/pose_graph_marginals/timing.json
    python scripts/pose_graph_marginals_timing.py --once     one optimize() and one fresh q = 4 call (to put under
                                                             rocprofv3 --kernel-trace --stats, in a run of its own)

Host clock with the device drained before and after each call (every call ends synchronised: it reads its result back)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import pose_graph_timing as T  # noqa: E402

REPEATS = 7


def queries(n):
    return {1: [n // 2], 4: [0, 959, 2000, n - 1], 40: [int(v) for v in np.linspace(0, n - 1, 40)]}


def main():
    import torch
    from lidar_slam_from_scratch_amd import build, capi
    from lidar_slam_from_scratch_amd import pose_graph as pg
    build.build_library()
    ctx = capi.Context(device=0)
    g = pg.PoseGraph(ctx)
    ops = T.kitti_ops()
    T.apply(g, ops)
    n = g.size()
    qs = queries(n)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    if "--once" in sys.argv:
        assert g.optimize()
        g.joint_marginal_covariance(qs[4])
        return
    assert g.optimize()                                    # warm-up: buffers, code objects
    g.joint_marginal_covariance(qs[40])
    out = {"poses": n, "loop_closures": g.loop_closure_count(), "repeats": REPEATS,
           "optimize_ms": 1e3 * statistics.median(timed(g.optimize) for _ in range(REPEATS))}
    for q, idx in qs.items():
        fresh, cached = [], []
        for _ in range(REPEATS):
            assert g.optimize()                            # clears the remembered factor
            fresh.append(timed(lambda: g.joint_marginal_covariance(idx)))
            cached.append(timed(lambda: g.joint_marginal_covariance(idx)))
        out["fresh_q%d_ms" % q] = 1e3 * statistics.median(fresh)
        out["cached_q%d_ms" % q] = 1e3 * statistics.median(cached)
    line = json.dumps(out)
    print(line)
    d = os.path.join(ROOT, "profiles", "pose_graph_marginals")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "timing.json"), "w") as f:
        f.write(line + "\n")
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
