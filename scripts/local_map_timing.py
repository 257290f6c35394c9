"""scripts/local_map_timing.py -- what the local map costs: host wall time, the device drained before and
after every timed call, of

    add         icpmi_local_map_add_device of one 64 x 1800 scan (voxel 0.5: ~10k rows, resident in device memory) into a
                table of ~30k rows (the drive's scans before it, under their true poses) and into one of ~200k rows
                (uniform points), each
                with the preparation of the new table as a target that the add queues behind its one wait (`add_ms` ends
                at the add's return, `add_and_prepare_ms` when the device is idle again)
    register    icpmi_local_map_register of the next scan against those tables: with the target the add prepared still
                remembered, and after an unrelated small registration made the context forget it
    per frame   odometry.run_odometry_local_map against odometry.run_odometry (frame-to-frame) on the same frames

The launch count of an add is a property of the code and of rocPRIM's choices for the scan's size, which this script
cannot see: LAUNCHES below is what `rocprofv3 --kernel-trace` of ten such adds showed, recorded with the timings.
Medians and every sample go to profiles/local_map/timing.json.  Nothing is asserted.

    python scripts/local_map_timing.py [--out profiles/local_map/timing.json] [--rounds 7] [--frames 12] [--table-frames 20]"""
import argparse
import json
import os
import statistics
import sys
import time

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: one HIP runtime per process)

from lidar_slam_from_scratch_amd import capi, odometry, synth  # noqa: E402
from lidar_slam_from_scratch_amd.local_map import LocalMap, LocalMapConfig  # noqa: E402

LAUNCHES = {"kernels": 10, "memsets": 1, "copies_back": 1,
            "chain": ["k_lmap_keys", "rocPRIM radix_sort_pairs: block sort + 4 block merges at 8.5k rows", "k_lmap_marks",
                      "rocPRIM exclusive_scan: scan-state init + scan", "k_lmap_merge"],
            "note": "from a kernel trace of ten adds of an 8,530-row scan: the same ten kernels into 15k and into 204k residents; the sort's "
                    "merge passes grow with the scan: 22 kernels for a 230k-row scan"}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return out, 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_ROOT, "profiles", "local_map", "timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--table-frames", type=int, default=20)
    args = ap.parse_args()

    tf = args.table_frames                                                    # the table; frame tf is added, frame tf + 1 registered
    n_frames = max(args.frames, tf + 2)
    frames = [synth.lidar_frame(f) for f in range(n_frames)]
    poses = [synth.lidar_pose(f) for f in range(n_frames)]
    rel = [synth.invert_transform(poses[0]) @ T for T in poses]
    rng = np.random.default_rng(5)
    big = np.stack([rng.uniform(-60.0, 60.0, 230000), rng.uniform(-60.0, 60.0, 230000), rng.uniform(-2.0, 6.0, 230000)], axis=1)
    other = synth.c3_uniform(3000, seed=71, perm_seed=72)[:2]                 # the unrelated registration that forgets

    ctx = capi.Context(device=0)
    config = LocalMapConfig()
    lmap = LocalMap(ctx, config)
    d_scan = torch.from_numpy(np.ascontiguousarray(frames[tf])).cuda()
    cfg = capi.Context.make_config(initial_transform=rel[tf + 1])
    small_cfg = capi.Context.make_config(max_iterations=2)
    out = {"voxel_size": config.voxel_size, "max_range": config.max_range, "rounds": args.rounds, "launches_per_add": LAUNCHES,
           "cases": {}}

    def build(case):
        lmap.clear()
        if case == "table_30k":
            for k in range(tf):
                lmap.add(frames[k], rel[k])
        else:
            lmap.add(big, np.eye(4))
        return lmap.size()

    for case in ("table_30k", "table_200k"):
        samples = []
        for r in range(args.rounds + 1):                                      # the first round warms up
            rows_before = build(case)
            info, add_ms, add_all_ms = wall_ms(lambda: lmap.add_device(d_scan.data_ptr(), d_scan.shape[0], rel[tf]))
            (res, _h), reg_ms, _ = wall_ms(lambda: lmap.register(frames[tf + 1], cfg))
            build(case)
            lmap.add_device(d_scan.data_ptr(), d_scan.shape[0], rel[tf])
            ctx.align(other[0], other[1], small_cfg)                          # the table's preparation is forgotten
            (res2, _h2), reg_cold_ms, _ = wall_ms(lambda: lmap.register(frames[tf + 1], cfg))
            assert res.num_iterations == res2.num_iterations and res.final_error == res2.final_error
            if r:
                samples.append({"add_ms": add_ms, "add_and_prepare_ms": add_all_ms, "register_remembered_ms": reg_ms,
                                "register_forgotten_ms": reg_cold_ms, "rows_before": rows_before, "rows_after": int(info.rows),
                                "inserted": int(info.inserted), "merged": int(info.merged), "dropped": int(info.dropped),
                                "passes": int(res.num_iterations)})
        med = {k: statistics.median(s[k] for s in samples) for k in ("add_ms", "add_and_prepare_ms", "register_remembered_ms",
                                                                     "register_forgotten_ms")}
        out["cases"][case] = {"scan_rows": int(d_scan.shape[0]), "rows_before": samples[0]["rows_before"],
                              "rows_after": samples[0]["rows_after"], "median": med, "samples": samples}
        print("%-10s scan %d rows into %d: add %.3f ms (%.3f with the preparation), register %.3f ms remembered, %.3f ms forgotten"
              % (case, d_scan.shape[0], samples[0]["rows_before"], med["add_ms"], med["add_and_prepare_ms"],
                 med["register_remembered_ms"], med["register_forgotten_ms"]))
    lmap.close()

    per_frame = {"local_map": [], "frame_to_frame": []}
    ate = {}
    frames, poses = frames[:args.frames], poses[:args.frames]
    for r in range(args.rounds + 1):
        a = odometry.run_odometry_local_map(frames, ctx, config)
        b = odometry.run_odometry(frames, odometry.gpu_align(ctx))
        if r:
            per_frame["local_map"].append(statistics.median(a.frame_ms))
            per_frame["frame_to_frame"].append(statistics.median(b.frame_ms))
        ate = {"local_map": odometry.absolute_trajectory_error(a, poses), "frame_to_frame": odometry.absolute_trajectory_error(b, poses),
               "local_map_passes": int(sum(a.iterations)), "frame_to_frame_passes": int(sum(b.iterations)), "map_rows": a.map_rows[-1]}
    out["odometry"] = {"frames": args.frames, "rows_per_frame": [int(f.shape[0]) for f in frames],
                       "median_frame_ms": {k: statistics.median(v) for k, v in per_frame.items()}, "samples": per_frame,
                       "ate_rms_m": ate}
    print("odometry, %d frames of 64 x 1800 (host clouds): local map %.3f ms per frame, frame-to-frame %.3f ms; ATE %.4f m against %.4f m"
          % (args.frames, out["odometry"]["median_frame_ms"]["local_map"], out["odometry"]["median_frame_ms"]["frame_to_frame"],
             ate["local_map"], ate["frame_to_frame"]))
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
