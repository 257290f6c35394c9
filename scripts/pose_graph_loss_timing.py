#!/usr/bin/env python3
"""What the loop-edge loss costs on the KITTI-00-shaped graph of scripts/pose_graph_timing.py (4,541 poses, 4,540
odometry factors, three closures per query on later laps): one optimize(), median of 7 after a warm-up,
    with the loss off            (the kernels of csrc/pose_graph.h; to set beside pose_graph_timing.py's figure)
    under Cauchy(1.0)            (csrc/pose_graph_loss.h), with its step and trial counts beside the time
and one loop_weights() call (one launch, one wait).

    python scripts/pose_graph_loss_timing.py [--out profiles/pose_graph_loss/timing.json]     one JSON line

Host clock around calls that end synchronised."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from pose_graph_timing import apply, kitti_ops  # noqa: E402


def timed(call, reps=7):
    call()                                           # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return {"ms_median": 1e3 * float(np.median(ts)), "ms_all": [round(1e3 * t, 3) for t in ts]}


def main():
    import torch  # noqa: F401
    from lidar_slam_from_scratch_amd import capi, pose_graph
    ops = kitti_ops()
    ctx = capi.Context(device=0)
    out = {"poses": 4541, "odometry": sum(o[0] == "odom" for o in ops), "closures": sum(o[0] == "loop" for o in ops)}
    for name, loss in (("loss_off", None), ("cauchy_1", (capi.PG_LOSS_CAUCHY, 1.0))):
        g = pose_graph.PoseGraph(ctx)
        if loss:
            g.set_loop_loss(*loss)
        apply(g, ops)

        def optimize():
            assert g.optimize()
        r = timed(optimize)
        st = g.stats
        r.update(iterations=st.iterations, inner_trials=st.inner_trials, stop_reason=st.stop_reason,
                 final_error=st.final_error, ms_per_trial=r["ms_median"] / st.inner_trials)
        w = timed(g.loop_weights)
        weights = g.loop_weights()[0]
        r.update(loop_weights_ms_median=w["ms_median"], loop_weights_ms_all=w["ms_all"],
                 least_weight=float(weights.min()))
        out[name] = r
        g.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
