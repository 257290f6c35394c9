"""Timing of the live counts (icpmi_map_live_update, csrc/live_counts.h) on scripts/map_timing.py's KITTI-00-shaped store:
4,541 frames of ~11k filtered points along a 3.7 km circle of poses, added one at a time as a node would.  One process:

    (a) per frame: icpmi_map_add_frame (not timed), then icpmi_map_live_update with one more pose (timed).  The medians
        over the 40 updates before the store holds 100, 1,000 and --frames frames; updates that moved the plane are
        listed apart (count, bytes copied, time)
    (b) the yardstick, what a node runs today for a live grid: icpmi_map_raycast_counts over the same store at those
        sizes (medians of --reps after a warm-up), and the ratio to (a)
    (c) a rebuild at --frames (icpmi_map_live_clear, then one update) against (b) at that size
    (d) n frames pending in one update, n = 1 .. 32, on the last frames of the store: per-frame kernels or the batch
        kernel, whichever the library under test takes
    (e) icpmi_map_live_counts (the copy out of the three arrays) at --frames
    (f) the device bytes the live state holds, from the buffer sizes

--lib PATH loads another build of the library (csrc/live_counts.h's ICPMI_LIVE_GROUPS and ICPMI_LIVE_BATCH_FRAMES are
compile-time constants; profiles/live/README.md says how the builds compared in profiles/live/tried.txt were made).
--device-only N adds N frames with one update each and nothing else (for rocprofv3 --kernel-trace --stats).

    python scripts/live_timing.py --out profiles/live/timing.json"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch  # noqa: F401  (first: one HIP runtime per process)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from map_timing import loop_poses, timed  # noqa: E402
from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402


def window_words(R):
    """ray_window_words (csrc/raycast.h)"""
    return (2 * R + 3) * ((2 * R + 3 + 62) // 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4541)
    ap.add_argument("--scans", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--device-only", type=int, default=0)
    ap.add_argument("--skip-yardstick", action="store_true", help="(a), (d) only: for the builds compared in tried.txt")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    L = capi.load_library(a.lib)
    from lidar_slam_from_scratch_amd.global_map import GlobalMap
    scans = [synth.lidar_frame(f, voxel=0.4) for f in range(0, 5 * a.scans, 5)]
    F = a.device_only or a.frames
    P = np.ascontiguousarray(np.stack(loop_poses(a.frames)))      # the same circle whatever F is: the prefix never moves
    dp = capi._dp(P)
    ctx = capi.Context(device=0)
    grid = capi.Context.make_grid_config()
    gm = GlobalMap(ctx)

    def update(n):
        info = capi.LiveInfo()
        ctx._check(L.icpmi_map_live_update(gm._h, dp, n, C.byref(grid), C.byref(info)))
        return info

    def batch(n):
        info = capi.CountsInfo()
        ctx._check(L.icpmi_map_raycast_counts(gm._h, dp, n, C.byref(grid), C.byref(info)))
        return info

    marks = sorted({m for m in (100, 1000, a.frames) if m <= F})
    res = {"frames": F, "lib": a.lib or "the tree's", "per_frame": {}, "yardstick": {}, "moves": []}
    times = np.zeros(F)
    for k in range(F):
        gm.add_frame(scans[k % len(scans)])
        t = time.perf_counter()
        info = update(k + 1)
        times[k] = time.perf_counter() - t
        assert info.frames_cast == 1 and info.rebuilt == 0
        if info.moved:
            res["moves"].append({"at": k + 1, "s": times[k], "box": [info.plane_w, info.plane_h]})
        if not a.device_only and not a.skip_yardstick and k + 1 in marks:
            s, all_s, b = timed(lambda: batch(k + 1), a.reps)
            assert bytes(b) == bytes(info.counts), "the live info is not the batch's"
            res["yardstick"][str(k + 1)] = {"s": s, "all": all_s}
    if a.device_only:
        return
    res["rows"] = gm.size()[1]
    moved_at = {m["at"] for m in res["moves"]}
    for m in marks:
        w = [times[k] for k in range(max(0, m - 40), m) if k + 1 not in moved_at]
        res["per_frame"][str(m)] = {"s": float(np.median(w)), "min": float(np.min(w)), "max": float(np.max(w)), "n": len(w)}
        if str(m) in res["yardstick"]:
            res["per_frame"][str(m)]["yardstick_over_live"] = res["yardstick"][str(m)]["s"] / res["per_frame"][str(m)]["s"]
    if len(marks) > 1:
        res["per_frame_last_over_first"] = res["per_frame"][str(marks[-1])]["s"] / res["per_frame"][str(marks[0])]["s"]
    # the bytes each move copied: the box before it (the first box is one frame's window)
    R = int(np.ceil(grid.max_range / grid.resolution))
    before = [2 * R + 3, 2 * R + 3]
    for m in res["moves"]:
        m["bytes_copied"] = 4 * before[0] * before[1]
        before = m["box"]
    res["moves_total"] = {"count": len(res["moves"]), "bytes": int(sum(m["bytes_copied"] for m in res["moves"])),
                          "s": float(sum(m["s"] for m in res["moves"])), "final_plane_bytes": 4 * info.plane_w * info.plane_h}
    print("per frame:", {m: "%.1f us" % (1e6 * v["s"]) for m, v in res["per_frame"].items()},
          "yardstick:", {m: "%.2f ms" % (1e3 * v["s"]) for m, v in res["yardstick"].items()}, flush=True)
    print("moves:", res["moves_total"], flush=True)

    # (d) n pending frames in one update: forget the last n (fewer poses: a rebuild of the rest, not timed), then add them
    res["pending"] = {}
    for n in (1, 2, 4, 8, 16, 32):
        ts = []
        for _ in range(a.reps):
            update(F - n)
            t = time.perf_counter()
            i = update(F)
            ts.append(time.perf_counter() - t)
            assert (i.frames_cast, i.rebuilt) == (n, 0) and bytes(i.counts) == bytes(info.counts)
        res["pending"][str(n)] = {"s": float(np.median(ts)), "all": ts, "moved": int(i.moved)}
    print("pending:", {n: "%.1f us" % (1e6 * v["s"]) for n, v in res["pending"].items()}, flush=True)

    if not a.skip_yardstick:
        def rebuild():
            ctx._check(L.icpmi_map_live_clear(gm._h))
            return update(F)
        res["rebuild_s"], res["rebuild_all"], i = timed(rebuild, a.reps)
        assert i.frames_cast == F and bytes(i.counts) == bytes(info.counts)
        res["rebuild_over_yardstick"] = res["rebuild_s"] / res["yardstick"][str(F)]["s"]
        res["live_counts_s"], res["live_counts_all"], c = timed(lambda: gm.live_counts()[0], a.reps)
        print("rebuild %.1f ms (%.2f of the batch call), live_counts %.1f ms" % (
            1e3 * res["rebuild_s"], res["rebuild_over_yardstick"], 1e3 * res["live_counts_s"]), flush=True)
        res["device_bytes"] = {"plane": 4 * i.plane_w * i.plane_h, "plane_cells": [i.plane_w, i.plane_h], "bounds": 40,
                               "windows": 8 * window_words(R), "arrays_after_live_counts": 5 * c.width * c.height,
                               "poses_host": 128 * F}
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("_all") and k != "moves"}))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    gm.close()
    ctx.close()


if __name__ == "__main__":
    main()
