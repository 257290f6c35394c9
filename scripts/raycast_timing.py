"""Timing of the ray-cast raster on scripts/map_timing.py's KITTI-00-shaped store: 4,541 frames of ~11k filtered
points, made from a few dozen synth.lidar_frame scans reused in turn along a 3.7 km circle of poses.

    (a) GlobalMap.raycast with the default grid (icpmi_map_raycast + the copy out, icpmi_map_raster)
    (b) icpmi_map_raycast alone (the raster stays on the device)
    (c) GlobalMap.finish with the grid and no published map: the cell set alone, the yardstick; and with the 1.0 m
        published map, the figure profiles/global_map records (icpmi_map_finish is the parent commit's, unchanged)
    (d) (b) at 0.25 m cells with max_range stretched: R at the LDS path's limit and one past it (the general path),
        and R = 351, 352 (the largest window within 64 KiB of LDS, and the next)
    (e) the CPU restatement (scripts/map_ref.py) on the first --cpu-frames frames; its raster is checked equal to the
        device's on the same frames

Medians of --reps runs after one warm-up ((e): one run).  --device-only runs (b) once (for rocprofv3 --kernel-trace
--stats).  The device memory the call allocates is worked out from the buffer sizes.

    python scripts/raycast_timing.py --out profiles/raycast/timing.json"""
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

    def raycast_only(g):
        info = capi.RasterInfo()
        ctx._check(L.icpmi_map_raycast(gm._h, capi._dp(P), P.shape[0], C.byref(g), C.byref(info)))
        return info

    if a.device_only:
        raycast_only(grid)
        return

    res = {"frames": frames, "rows": rows, "reps": a.reps}
    res["a_raycast_and_copy_s"], res["a_all"], raster = timed(lambda: gm.raycast(poses, grid), a.reps)
    res["b_raycast_s"], res["b_all"], info = timed(lambda: raycast_only(grid), a.reps)
    res["c_finish_cells_s"], res["c_all"], (cells, _) = timed(lambda: gm.finish(poses, grid, 0.0), a.reps)
    res["c_finish_full_s"], res["c_full_all"], _ = timed(lambda: gm.finish(poses, grid, 1.0), a.reps)   # profiles/global_map's (b)
    res["ratio_b_over_c"] = res["b_raycast_s"] / res["c_finish_cells_s"]
    print("(a) %.1f ms  (b) %.1f ms  (c) %.1f ms, %.1f ms with the published map" % (
        1e3 * res["a_raycast_and_copy_s"], 1e3 * res["b_raycast_s"], 1e3 * res["c_finish_cells_s"],
        1e3 * res["c_finish_full_s"]), flush=True)
    res["raster"] = {"min_x": info.min_x, "min_y": info.min_y, "width": info.width, "height": info.height,
                     "n_occupied": info.n_occupied, "n_free": info.n_free}
    y, x = np.nonzero(raster.data == 100)
    order = np.lexsort((y, x))
    res["occupied_equals_finish"] = bool(np.array_equal(np.stack([x + raster.min_x, y + raster.min_y], axis=1)[order], cells))

    res["d"] = {}
    for R in (351, 352, capi.RAYCAST_LDS_MAX_R, capi.RAYCAST_LDS_MAX_R + 1):   # 351: the largest window within 64 KiB
        g = capi.Context.make_grid_config(resolution=0.25, max_range=0.25 * R)
        t, ts, i = timed(lambda: raycast_only(g), a.reps)
        res["d"]["R=%d" % R] = {"s": t, "all": ts, "n_free": i.n_free, "n_occupied": i.n_occupied}
        print("(d) R = %d: %.1f ms" % (R, 1e3 * t), flush=True)

    # the call's device memory, from its buffer sizes (csrc/capi.hip, icpmi_map_raycast)
    Rc = int(np.ceil(grid.max_range / grid.resolution))
    sensors = np.floor(P[:, :2, 3] / grid.resolution)
    W, H = (int(v) + 2 * Rc + 3 for v in sensors.max(axis=0) - sensors.min(axis=0))
    res["device_bytes"] = {"keys": 8 * rows, "frame_table": 24 * frames, "two_bit_planes": 2 * 4 * ((W + 31) // 32) * H,
                           "raster": info.width * info.height, "plane_cells": [W, H]}

    n = min(a.cpu_frames, frames)
    ref = map_ref.MapRef()
    for k in range(n):
        ref.add_frame(scans[k % len(scans)])
    res["e_cpu_frames"], res["e_cpu_rows"] = n, ref.size()[1]
    res["e_cpu_s"], _, want = timed(lambda: ref.raycast(poses[:n], grid), 1, warm=False)
    got = gm.raycast(poses[:n], grid)
    res["equal_e"] = bool((got.min_x, got.min_y, got.width, got.height, got.n_occupied, got.n_free) ==
                          (want.min_x, want.min_y, want.width, want.height, want.n_occupied, want.n_free) and
                          np.array_equal(got.data, want.data))
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
