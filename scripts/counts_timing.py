"""Timing of the hit / miss counts on scripts/map_timing.py's KITTI-00-shaped store: 4,541 frames of ~11k filtered
points, made from a few dozen synth.lidar_frame scans reused in turn along a 3.7 km circle of poses.  One process:

    (a) icpmi_map_raycast_counts with the default grid (the arrays stay on the device)
    (b) icpmi_map_raycast, the yardstick: its code is untouched by the counts
    (c) GlobalMap.raycast_counts: (a) and the copy out of the three arrays (icpmi_map_counts)
    (d) (a) at 0.25 m cells with max_range stretched: R = 392 (the largest pair of windows LDS takes) and 393 (the
        windows in device scratch), and R = 239, 240 (the largest pair within 64 KiB of LDS, and the next)
    (e) the CPU restatement (scripts/map_ref.py) on the first --cpu-frames frames; its arrays are checked equal to
        the device's on the same frames

Medians of --reps runs after one warm-up ((e): one run).  --device-only runs (a) once (for rocprofv3 --kernel-trace
--stats).  The count adds issued are the sum over frames of |H_i| + |C_i|, which is the sum of both arrays; the
device memory the call allocates is worked out from the buffer sizes.

    python scripts/counts_timing.py --out profiles/raycast_counts/timing.json"""
import argparse
import ctypes as C
import json
import os
import sys

import torch  # noqa: F401  (first: one HIP runtime per process)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import map_ref  # noqa: E402
from map_timing import loop_poses, timed  # noqa: E402
from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402
from lidar_slam_from_scratch_amd.global_map import GlobalMap  # noqa: E402


def window_words(R):
    """ray_window_words (csrc/raycast.h)"""
    return (2 * R + 3) * ((2 * R + 3 + 62) // 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4541)
    ap.add_argument("--scans", type=int, default=24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-frames", type=int, default=200)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    scans = [synth.lidar_frame(f, voxel=0.4) for f in range(0, 5 * a.scans, 5)]
    poses = loop_poses(a.frames)
    ctx = capi.Context(device=0)
    L = capi.load_library()
    grid = capi.Context.make_grid_config()
    gm = GlobalMap(ctx)
    for k in range(a.frames):
        gm.add_frame(scans[k % len(scans)])
    frames, rows = gm.size()
    print("store: %d frames, %d rows (%.1f per frame)" % (frames, rows, rows / frames), flush=True)
    P = np.ascontiguousarray(np.stack(poses))

    def counts_only(g):
        info = capi.CountsInfo()
        ctx._check(L.icpmi_map_raycast_counts(gm._h, capi._dp(P), P.shape[0], C.byref(g), C.byref(info)))
        return info

    def raycast_only(g):
        info = capi.RasterInfo()
        ctx._check(L.icpmi_map_raycast(gm._h, capi._dp(P), P.shape[0], C.byref(g), C.byref(info)))
        return info

    if a.device_only:
        counts_only(grid)
        return

    res = {"frames": frames, "rows": rows, "reps": a.reps}
    res["a_counts_s"], res["a_all"], info = timed(lambda: counts_only(grid), a.reps)
    res["b_raycast_s"], res["b_all"], rinfo = timed(lambda: raycast_only(grid), a.reps)
    res["c_counts_and_copy_s"], res["c_all"], counts = timed(lambda: gm.raycast_counts(poses, grid), a.reps)
    res["ratio_a_over_b"] = res["a_counts_s"] / res["b_raycast_s"]
    print("(a) %.1f ms  (b) %.1f ms  (c) %.1f ms  a / b = %.2f" % (
        1e3 * res["a_counts_s"], 1e3 * res["b_raycast_s"], 1e3 * res["c_counts_and_copy_s"], res["ratio_a_over_b"]), flush=True)
    res["counts"] = {f: getattr(info, f) for f, _ in capi.CountsInfo._fields_ if f != "pad"}
    res["same_box_as_raycast"] = bool((info.min_x, info.min_y, info.width, info.height, info.n_hit_cells, info.n_observed) ==
                                      (rinfo.min_x, rinfo.min_y, rinfo.width, rinfo.height, rinfo.n_occupied,
                                       rinfo.n_occupied + rinfo.n_free))
    res["count_adds"] = {"hits": int(counts.hits.sum(dtype=np.uint64)), "misses": int(counts.misses.sum(dtype=np.uint64))}
    res["count_adds"]["all"] = res["count_adds"]["hits"] + res["count_adds"]["misses"]
    print("count adds: %d" % res["count_adds"]["all"], flush=True)

    res["d"] = {}
    for R in (239, 240, capi.RAYCOUNT_LDS_MAX_R, capi.RAYCOUNT_LDS_MAX_R + 1):
        g = capi.Context.make_grid_config(resolution=0.25, max_range=0.25 * R)
        t, ts, i = timed(lambda: counts_only(g), a.reps)
        res["d"]["R=%d" % R] = {"s": t, "all": ts, "n_observed": i.n_observed, "n_hit_cells": i.n_hit_cells,
                                "max_hits": i.max_hits, "max_misses": i.max_misses}
        print("(d) R = %d: %.1f ms" % (R, 1e3 * t), flush=True)

    # the call's device memory, from its buffer sizes (csrc/capi.hip, icpmi_map_raycast_counts)
    Rc = int(np.ceil(grid.max_range / grid.resolution))
    sensors = np.floor(P[:, :2, 3] / grid.resolution)
    W, H = (int(v) + 2 * Rc + 3 for v in sensors.max(axis=0) - sensors.min(axis=0))
    res["device_bytes"] = {"keys": 8 * rows, "frame_table": 24 * frames, "count_plane": 4 * W * H,
                           "arrays": 5 * info.width * info.height, "plane_cells": [W, H],
                           "lds_window_pair": 8 * window_words(Rc),
                           "scratch_windows_at_R=393": 8 * window_words(393) * min(256, frames)}

    n = min(a.cpu_frames, frames)
    ref = map_ref.MapRef()
    for k in range(n):
        ref.add_frame(scans[k % len(scans)])
    res["e_cpu_frames"], res["e_cpu_rows"] = n, ref.size()[1]
    res["e_cpu_s"], _, want = timed(lambda: ref.raycast_counts(poses[:n], grid), 1, warm=False)
    got = gm.raycast_counts(poses[:n], grid)
    fields = ("min_x", "min_y", "width", "height", "n_observed", "n_hit_cells", "max_hits", "max_misses", "frames_used")
    res["equal_e"] = bool(all(getattr(got, f) == getattr(want, f) for f in fields) and np.array_equal(got.hits, want.hits) and
                          np.array_equal(got.misses, want.misses) and np.array_equal(got.probability, want.probability))
    print("(e) %.2f s on %d frames, equal: %s" % (res["e_cpu_s"], n, res["equal_e"]), flush=True)
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("_all")}))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    gm.close()
    ctx.close()


if __name__ == "__main__":
    main()
