#!/usr/bin/env python3
"""What information edges cost on the KITTI-00-shaped graph of scripts/pose_graph_timing.py (4,541 poses, 4,540
odometry factors, three closures per query on later laps): one optimize(), median of 7 after a warm-up,
    diagonal          every edge under the config's sigmas (the kernels of csrc/pose_graph.h; to set beside
                      pose_graph_timing.py's figure on the parent commit)
    information       every between factor an information edge with L = diag(1 / sigma^2) of the sigmas it had: the same
                      problem through k_pg_linearize_info / k_pg_trial_info (csrc/pose_graph_info.h), so that the step
                      counts agree and the times compare
    mixed             the closures as information edges, the odometry diagonal
and the time the 4,900 add calls take on the host, where the information is factored.

    python scripts/pose_graph_info_timing.py [--out profiles/pose_graph_info/timing.json]     one JSON line

Host clock around calls that end synchronised."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import pose_graph_info_ref as I  # noqa: E402
from pose_graph_timing import kitti_ops  # noqa: E402


def as_information(ops, cfg, which):
    out = []
    for op in ops:
        if op[0] == "odom" and "odom" in which:
            s = 1.0 + 10.0 * op[4]
            sig = np.array([cfg.odom_rotation_sigma * s] * 3 + [cfg.odom_translation_sigma * s] * 3)
            out.append(("odom_info", op[1], op[2], op[3], np.diag(1.0 / sig ** 2)))
        elif op[0] == "loop" and "loop" in which:
            sig = np.array([cfg.loop_rotation_sigma] * 3 + [cfg.loop_translation_sigma] * 3)
            out.append(("loop_info", op[1], op[2], op[3], np.diag(1.0 / sig ** 2)))
        else:
            out.append(op)
    return out


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
    poses = {}
    for name, which in (("diagonal", ()), ("information", ("odom", "loop")), ("mixed", ("loop",))):
        g = pose_graph.PoseGraph(ctx)
        mine = as_information(ops, g.config, which)
        t0 = time.perf_counter()
        I.apply(g, mine)
        add_ms = 1e3 * (time.perf_counter() - t0)

        def optimize():
            assert g.optimize()
        r = timed(optimize)
        st = g.stats
        r.update(iterations=st.iterations, inner_trials=st.inner_trials, stop_reason=st.stop_reason,
                 final_error=st.final_error, ms_per_trial=r["ms_median"] / st.inner_trials, add_calls_ms=add_ms,
                 information_factors=sum(o[0].endswith("_info") for o in mine))
        poses[name] = np.stack(g.get_all_poses())
        out[name] = r
        g.close()
    ctx.close()
    out["largest_pose_difference_information_vs_diagonal"] = float(np.abs(poses["information"] - poses["diagonal"]).max())
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
