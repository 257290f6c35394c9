"""Timing of loop-closure detection on the KITTI-00-shaped store of scripts/map_timing.py (4,541 frames of ~11k filtered
points made from a few dozen reused synth.lidar_frame scans): the host detector (loop_closure.LoopClosureDetector over
GpuBackend, which keeps every cloud and descriptor on the host) against the store detector (StoreLoopClosureDetector,
whose database lives on the device as an index over the store's frames), both in the same process on the same context.

The store reuses --scans scans in turn, so each query has an exact copy every --scans frames: far more candidates than
KITTI (every copy at least frame_gap back passes the threshold).  max_candidates = 3 caps the verifications.

    (a) one detect for the newest of N entries (N = 100, 1,000, 4,540): the candidate phase alone (max_candidates = 0)
        and the whole detect (the node's config); verifications = whole - candidate phase
    (b) the per-frame add: host add_frame(cloud) against store add_frame(store_frame) (+ the descriptor, formed in the
        next detect's first launch: (c) carries it)
    (c) the node's whole pattern: add every registered frame 1 .. F-1, detect at k % 10 == 0, k > 50 (449 detects)

Medians of --reps runs after one warm-up, with min and max.  (c) also checks that both detectors return the same
closures bit for bit.  --device-only runs (c) for the store detector alone (for rocprofv3).

--yaw-guess measures the yaw guess instead, in one process:
    (d) the candidate phase (max_candidates = 0) of one detect for the newest of N entries, k_loop_candidates and
        k_loop_candidates_shift alternating call by call on two detectors over the same store
    (e) the verifications of scripts/loop_yaw_ref.py's reverse drive R12 through the host detector, from the identity and
        from the shift: how many, their iteration counts, their summed time, the closures accepted

    python scripts/loop_store_timing.py --out profiles/loop_store/timing.json
    python scripts/loop_store_timing.py --yaw-guess --out profiles/loop_store/yaw_timing.json"""
import argparse
import json
import os
import sys
import time

import torch  # noqa: F401  (first: one HIP runtime per process)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402
from lidar_slam_from_scratch_amd import loop_closure as lc  # noqa: E402
from lidar_slam_from_scratch_amd.global_map import GlobalMap  # noqa: E402
from lidar_slam_from_scratch_amd.slam import node_loop_config  # noqa: E402


def stats(ts):
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)), "max_ms": 1e3 * float(np.max(ts)),
            "n": len(ts)}


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return stats(ts)


def cfg(max_candidates):
    c = node_loop_config()
    c.max_candidates = max_candidates
    return c


def same(a, b):
    u = lambda v: np.asarray(v, dtype=np.float64).view(np.uint64)  # noqa: E731
    return len(a) == len(b) and all(
        (x.query_frame, x.match_frame) == (y.query_frame, y.match_frame) and u([x.scan_context_distance]) == u([y.scan_context_distance])
        and u([x.icp_fitness]) == u([y.icp_fitness]) and np.array_equal(u(x.transform), u(y.transform)) for x, y in zip(a, b))


def node_pattern(det, frames, add):
    out = []
    for k in range(1, frames):
        add(det, k)
        if k % 10 == 0 and k > 50:
            out += det.detect()
    return out


class TimedBackend(lc.GpuBackend):
    """GpuBackend that records every verification's iteration count and the time spent in them"""

    def __init__(self, ctx):
        super().__init__(ctx)
        self.iterations, self.seconds = [], 0.0

    def align(self, *args, **kw):
        t = time.perf_counter()
        r = super().align(*args, **kw)
        self.seconds += time.perf_counter() - t
        self.iterations.append(int(r.num_iterations))
        return r

    def align_many(self, *args, **kw):
        t = time.perf_counter()
        rs = super().align_many(*args, **kw)
        self.seconds += time.perf_counter() - t
        self.iterations += [int(r.num_iterations) for r in rs]
        return rs


def yaw_guess_timing(ctx, gm, sizes, reps):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import loop_yaw_ref as ref
    res = {"candidates": {}, "reverse_drive": {}}
    for n in sizes:
        dets = {}
        for on in (False, True):
            c = cfg(0)
            c.yaw_guess = on
            dets[on] = lc.StoreLoopClosureDetector(ctx, gm, c)
            for k in range(n):
                dets[on].add_frame(k, k)
            dets[on].detect()                                   # the descriptors, and a warm-up
        ts = {False: [], True: []}
        for _ in range(reps):
            for on in (False, True):                            # alternating, call by call
                t = time.perf_counter()
                dets[on].detect()
                ts[on].append(time.perf_counter() - t)
        res["candidates"][str(n)] = {"k_loop_candidates": stats(ts[False]), "k_loop_candidates_shift": stats(ts[True])}
        for d in dets.values():
            d.close()
        print(n, json.dumps({k: v["median_ms"] for k, v in res["candidates"][str(n)].items()}), flush=True)
    poses, labels = ref.r12_reverse_drive()
    clouds = ref.scans(poses)
    for on in (False, True):
        for rep in range(2):                                    # the second pass is the one kept (the first warms up)
            be = TimedBackend(ctx)
            det = lc.LoopClosureDetector(be, lc.LoopClosureConfig(frame_gap=50, sc_distance_threshold=0.2,
                                                                  icp_fitness_threshold=0.3, yaw_guess=on))
            found = []
            for c, label in zip(clouds, labels):
                det.add_frame(c, label)
                found += det.detect()
        res["reverse_drive"]["on" if on else "off"] = {
            "verifications": len(be.iterations), "iterations": be.iterations, "verify_ms": 1e3 * be.seconds,
            "closures": [(r.query_frame, r.match_frame, r.sector_shift) for r in found]}
        print("reverse drive, guess %s: %s" % ("on" if on else "off", json.dumps(res["reverse_drive"]["on" if on else "off"])),
              flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4541)
    ap.add_argument("--scans", type=int, default=24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="100,1000,4540")
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--yaw-guess", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    scans = [synth.lidar_frame(f, voxel=0.4) for f in range(0, 5 * a.scans, 5)]
    cloud = lambda k: scans[k % len(scans)]  # noqa: E731
    ctx = capi.Context(device=0)
    gm = GlobalMap(ctx)
    for k in range(a.frames):
        gm.add_frame(cloud(k))
    frames, rows = gm.size()
    print("store: %d frames, %d rows (%.1f per frame)" % (frames, rows, rows / frames), flush=True)
    add_host = lambda d, k: d.add_frame(cloud(k), k)  # noqa: E731
    add_dev = lambda d, k: d.add_frame(k, k)  # noqa: E731
    if a.yaw_guess:
        res = yaw_guess_timing(ctx, gm, [int(s) for s in a.sizes.split(",")], a.reps)
        res.update(frames=frames, rows=rows, reps=a.reps)
        if a.out:
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        gm.close()
        ctx.close()
        return
    if a.device_only:
        t = time.perf_counter()
        r = node_pattern(lc.StoreLoopClosureDetector(ctx, gm, cfg(3)), frames, add_dev)
        print("store detector, node pattern: %.1f ms, %d closures" % (1e3 * (time.perf_counter() - t), len(r)))
        return

    res = {"frames": frames, "rows": rows, "scans": a.scans, "reps": a.reps, "detect": {}}
    for n in [int(s) for s in a.sizes.split(",")]:
        row = {}
        for name, make, add in (("host", lambda c: lc.LoopClosureDetector(lc.GpuBackend(ctx), c), add_host),
                                ("store", lambda c: lc.StoreLoopClosureDetector(ctx, gm, c), add_dev)):
            for mc, key in ((0, "candidates"), (3, "whole")):
                d = make(cfg(mc))
                for k in range(n):
                    add(d, k)
                row["%s_%s" % (name, key)] = timed(d.detect, a.reps)
                if mc == 3:
                    row["%s_closures" % name] = len(d.detect())
                if name == "store":
                    d.close()
                del d
            row["%s_verify_median_ms" % name] = row["%s_whole" % name]["median_ms"] - row["%s_candidates" % name]["median_ms"]
        res["detect"][str(n)] = row
        print(n, json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)

    hd = lc.LoopClosureDetector(lc.GpuBackend(ctx), cfg(3))
    sd = lc.StoreLoopClosureDetector(ctx, gm, cfg(3))
    ts_h, ts_s = [], []
    for k in range(200):
        t = time.perf_counter()
        add_host(hd, k)
        ts_h.append(time.perf_counter() - t)
        t = time.perf_counter()
        add_dev(sd, k)
        ts_s.append(time.perf_counter() - t)
    res["add_host"], res["add_store"] = stats(ts_h), stats(ts_s)
    sd.close()
    print("add: host %.3f ms, store %.4f ms" % (res["add_host"]["median_ms"], res["add_store"]["median_ms"]), flush=True)

    outs = {}
    for name, make, add in (("host", lambda: lc.LoopClosureDetector(lc.GpuBackend(ctx), cfg(3)), add_host),
                            ("store", lambda: lc.StoreLoopClosureDetector(ctx, gm, cfg(3)), add_dev)):
        d = make()
        t = time.perf_counter()
        outs[name] = node_pattern(d, frames, add)
        res["node_%s_s" % name] = time.perf_counter() - t
        if name == "store":
            d.close()
        del d
        print("node pattern, %s: %.2f s, %d closures" % (name, res["node_%s_s" % name], len(outs[name])), flush=True)
    res["node_detects"] = sum(1 for k in range(1, frames) if k % 10 == 0 and k > 50)
    res["node_closures"] = len(outs["store"])
    res["node_equal"] = bool(same(outs["host"], outs["store"]))
    res["node_speedup"] = res["node_host_s"] / res["node_store_s"]
    print(json.dumps({k: v for k, v in res.items() if k != "detect"}))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    gm.close()
    ctx.close()


if __name__ == "__main__":
    main()
