"""Timing of the static published map (icpmi_map_finish_static, csrc/static_map.h) next to the two calls it replaces
for a node that wants both the live counts and a published map: icpmi_map_live_update followed by icpmi_map_finish's
published-map half (grid NULL).  The store is scripts/static_map_ref.py's moving-car drive extended to --frames frames
(40: about 270k rows), the grid the drive's, the rule the default one, the voxel 1.0.  Two cases, each the median of
--reps timed calls after one warm-up, with the range:

    nothing_new   every frame is cast already: the live update inside the call has nothing to do
    one_new       the last frame is new.  Before each timed call an update over one frame fewer rebuilds the live counts
                  (not timed); the timed call then casts the one frame

What is timed is the WALL time of a call from the host, which ends in the call's last wait for the device and includes
the copy of the result to the host: the library does not hand out its stream, so no HIP events bracket the queue from
here.  The two new kernels on their own are not timed, and neither are real scans.

    python scripts/static_map_timing.py --out profiles/static_map/timing.json"""
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

import static_map_ref as ref  # noqa: E402
from lidar_slam_from_scratch_amd import capi  # noqa: E402
from lidar_slam_from_scratch_amd.global_map import GlobalMap  # noqa: E402


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(np.min(ts)), "max_s": float(np.max(ts)), "all_s": [float(t) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--voxel", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    clouds, poses, grid, _, _ = ref.moving_car_drive(frames=a.frames)
    L = capi.load_library()
    ctx = capi.Context(device=0)
    gm = GlobalMap(ctx)
    for c in clouds:
        gm.add_frame(c)
    F, rows = gm.size()
    g = capi.Context.make_grid_config(**grid)
    rule = capi.StaticRule()
    P = np.ascontiguousarray(np.stack(poses))
    dp = capi._dp(P)
    out = np.empty((rows, 3))
    nm, si, li = C.c_int64(0), capi.StaticInfo(), capi.LiveInfo()

    def finish_static(n):
        ctx._check(L.icpmi_map_finish_static(gm._h, dp, n, C.byref(g), C.byref(rule), a.voxel, capi._dp(out), rows, C.byref(nm), C.byref(si)))

    def live_update(n):
        ctx._check(L.icpmi_map_live_update(gm._h, dp, n, C.byref(g), C.byref(li)))

    def finish_published(n):
        ctx._check(L.icpmi_map_finish(gm._h, dp, n, None, a.voxel, capi._dp(out), rows, C.byref(nm), None))

    def parent_pair(n):
        live_update(n)
        finish_published(n)

    def timed(fn, before, check):
        ts = []
        for rep in range(a.reps + 1):                                     # the first is the warm-up
            before()
            t = time.perf_counter()
            fn(F)
            dt = time.perf_counter() - t
            check()
            if rep:
                ts.append(dt)
        return stats(ts)

    res = {"frames": F, "rows": rows, "grid": grid, "rule": [rule.min_probability, rule.min_observations], "voxel": a.voxel,
           "reps": a.reps, "what": "wall time of the whole call from the host, its waits and the copy out included"}
    live_update(F)

    def nothing():
        pass

    def forget_last():
        live_update(F - 1)                                                # fewer poses: a rebuild of the rest

    def cast(k, info):
        def check():
            assert (info().frames_cast, info().rebuilt) == (k, 0), (info().frames_cast, info().rebuilt)
        return check

    res["nothing_new"] = {"finish_static": timed(finish_static, nothing, cast(0, lambda: si.live)),
                          "live_update_then_finish": timed(parent_pair, nothing, cast(0, lambda: li)),
                          "finish_alone": timed(finish_published, nothing, nothing)}
    res["one_new"] = {"finish_static": timed(finish_static, forget_last, cast(1, lambda: si.live)),
                      "live_update_then_finish": timed(parent_pair, forget_last, cast(1, lambda: li))}
    finish_static(F)
    res["static_info"] = {"rows": si.rows, "voting": si.voting, "dropped": si.dropped, "kept": si.kept, "published_rows": nm.value}
    finish_published(F)
    res["published_rows_plain"] = nm.value
    for case in ("nothing_new", "one_new"):
        r = res[case]
        r["static_over_pair"] = r["finish_static"]["median_s"] / r["live_update_then_finish"]["median_s"]
        print("%s: finish_static %.2f ms (%.2f .. %.2f), live_update + finish %.2f ms (%.2f .. %.2f)" % (
            case, 1e3 * r["finish_static"]["median_s"], 1e3 * r["finish_static"]["min_s"], 1e3 * r["finish_static"]["max_s"],
            1e3 * r["live_update_then_finish"]["median_s"], 1e3 * r["live_update_then_finish"]["min_s"],
            1e3 * r["live_update_then_finish"]["max_s"]), flush=True)
    print(json.dumps({k: v for k, v in res.items() if k not in ("nothing_new", "one_new")}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    gm.close()
    ctx.close()


if __name__ == "__main__":
    main()
