"""Timing of the global map on a KITTI-00-shaped store: 4,541 frames of ~15k filtered points, made from a few dozen
synth.lidar_frame scans reused in turn along a KITTI-sized loop of poses (a circle of ~3.7 km).

    (a) recent clouds: GlobalMap.recent_clouds (icpmi_map_world, last 20 frames)
    (b) GlobalMap.finish: the cell set rebuilt and the 1.0 m published map (icpmi_map_finish)
    (c) the same result through the calls that existed before: per frame transform_points + occupancy_update, then
        voxel_downsample of the host-concatenated map
    (d) the CPU restatement (scripts/map_ref.py)

Medians of --reps runs after one warm-up ((d): --cpu-reps runs, no warm-up).  Every leg's outputs are checked equal.
--device-only runs (a) and (b) once each (for rocprofv3 --kernel-trace --stats).

    python scripts/map_timing.py --out profiles/global_map/timing.json"""
import argparse
import json
import os
import sys
import time

import torch  # noqa: F401  (first: one HIP runtime per process)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import map_ref  # noqa: E402
from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402
from lidar_slam_from_scratch_amd.global_map import GlobalMap  # noqa: E402


def loop_poses(F, length=3700.0):
    r = length / (2 * np.pi)
    P = []
    for k in range(F):
        a = 2 * np.pi * k / F
        P.append(synth.make_transform([0.0, 0.0, a + np.pi / 2], [r * np.cos(a), r * np.sin(a), 0.0]))
    return P


def timed(fn, reps, warm=True):
    if warm:
        fn()
    ts, out = [], None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), ts, out


def row_set(a):
    u = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3).view(np.uint64)
    return u[np.lexsort(u.T[::-1])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4541)
    ap.add_argument("--scans", type=int, default=24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-reps", type=int, default=1)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    scans = [synth.lidar_frame(f, voxel=0.4) for f in range(0, 5 * a.scans, 5)]
    poses = loop_poses(a.frames)
    ctx = capi.Context(device=0)
    grid = capi.Context.make_grid_config()
    gm = GlobalMap(ctx)
    for k in range(a.frames):
        gm.add_frame(scans[k % len(scans)])
    frames, rows = gm.size()
    print("store: %d frames, %d rows (%.1f per frame)" % (frames, rows, rows / frames), flush=True)
    if a.device_only:
        gm.recent_clouds(poses)
        gm.finish(poses, grid, 1.0)
        return

    res = {"frames": frames, "rows": rows, "reps": a.reps}
    res["a_recent_s"], res["a_all"], _ = timed(lambda: gm.recent_clouds(poses), a.reps)
    res["b_finish_s"], res["b_all"], (cells_b, map_b) = timed(lambda: gm.finish(poses, grid, 1.0), a.reps)
    print("(a) %.2f ms  (b) %.1f ms" % (1e3 * res["a_recent_s"], 1e3 * res["b_finish_s"]), flush=True)

    def today():
        ctx.occupancy_clear()
        worlds = []
        for k in range(a.frames):
            w = ctx.transform_points(poses[k], scans[k % len(scans)])
            ctx.occupancy_update(w, poses[k][:3, 3], grid)
            worlds.append(w)
        published = ctx.voxel_downsample(np.concatenate(worlds), 1.0)
        return ctx.occupancy_cells(), published

    res["c_today_s"], res["c_all"], (cells_c, map_c) = timed(today, a.reps)
    print("(c) %.1f ms" % (1e3 * res["c_today_s"]), flush=True)

    ref = map_ref.MapRef()
    for k in range(a.frames):
        ref.add_frame(scans[k % len(scans)])
    res["d_cpu_s"], res["d_all"], (cells_d, map_d) = timed(lambda: ref.finish(poses, grid, 1.0), a.cpu_reps, warm=False)
    print("(d) %.1f ms" % (1e3 * res["d_cpu_s"]), flush=True)

    res["cells"], res["published_rows"] = int(len(cells_b)), int(len(map_b))
    res["equal_b_c"] = bool(np.array_equal(cells_b, cells_c) and np.array_equal(row_set(map_b), row_set(map_c)))
    res["equal_b_d"] = bool(np.array_equal(cells_b, cells_d) and np.array_equal(row_set(map_b), row_set(map_d)))
    recent = gm.recent_clouds(poses)
    want = ref.recent_clouds(poses)
    res["equal_a_d"] = bool(len(recent) == len(want) and all(
        np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(recent, want)))
    res["speedup_b_vs_c"] = res["c_today_s"] / res["b_finish_s"]
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("_all")}))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    gm.close()
    ctx.close()


if __name__ == "__main__":
    main()
