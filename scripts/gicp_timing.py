"""scripts/gicp_timing.py -- what the plane-to-plane cost costs per pass: device time of the iteration loop
(HIP events around it, icpmi_profile.loop_ms) of icpmi_align_gicp (epsilon 1e-3 behind the 2 m gate) against
icpmi_align_gated at the same gate on the same pairs,

    l12_6_5       an L12 pair (4,342 -> 4,372 rows) from its verification's start: gated the small-cloud kernel,
                  plane-to-plane the general path (search + k_reduce_gicp + k_finish_step_gated + k_transform) and, third,
                  plane-to-plane in its small form (ICPMI_GICP_FORM_SMALL: k_icp_small_gicp + k_finish_step_gated)
    c3_20k        20,000 -> 20,000 uniform points: both the general path, k_reduce_gated against k_reduce_gicp
    c3_100k       100,000 -> 100,000

with tolerance 0 and min_error 0, so that all run exactly max_iterations passes and the post-loop one.  The forms
alternate on one context, seven rounds after a warm-up of each; the medians and every sample go to
profiles/gicp/timing.json.  The gated kernels and the general plane-to-plane path are unchanged by the small form, so
they are its baseline.  (The small form is timed where it runs, on l12_6_5; on the two larger pairs the flag has no effect.)
Last, the wall time of every detect() of the L12 drive through the store detector (yaw guess, 2 m gate), summed, under the
gate alone, Huber 0.1 m and plane-to-plane epsilon = 1e-3: the three alternate, --detect-rounds drives each after a warm-up.  The call's
fixed part is the call's device time less the loop's (total_ms - loop_ms): the plane-to-plane call's holds the source's
search structure and 20-NN normals on top of the target's.  Only the loop and the call are timed (profile = 1): the
kernels' own times, k_reduce_gicp against k_reduce_gated among them, are not taken here.  Nothing is asserted.

    python scripts/gicp_timing.py [--out profiles/gicp/timing.json] [--rounds 7] [--iterations 20] [--detect-rounds 5]"""
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

import torch  # noqa: F401,E402  (first: one HIP runtime per process)

import gated_icp_ref as gr  # noqa: E402
import gicp_ref as ref  # noqa: E402
from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402

FORMS = ("gated", "gicp")
SMALL_CASES = ("l12_6_5",)    # where the small-cloud kernel runs: the third form, "gicp_small", is timed there
DETECT_MODES = ("gate", "huber", "gicp")


def detect_wall(ctx, clouds, labels, mode):
    """-> (seconds in detect() over the L12 drive, closures, small-cloud launches): the store detector, yaw guess, 2 m gate"""
    from lidar_slam_from_scratch_amd import loop_closure as lc
    from lidar_slam_from_scratch_amd.global_map import GlobalMap
    import robust_icp_ref as rr
    kw = dict(gr.L12_CONFIG, yaw_guess=True, max_correspondence_distance=gr.L12_GATE)
    if mode == "huber":
        kw.update(robust_kind=rr.HUBER, robust_scale=rr.HUBER_SCALE)
    elif mode == "gicp":
        kw.update(gicp_epsilon=ref.EPSILON_DEFAULT)
    store = GlobalMap(ctx)
    det = lc.StoreLoopClosureDetector(ctx, store, lc.LoopClosureConfig(**kw))
    ctx.reset_profile()
    spent, found = 0.0, 0
    for cloud, label in zip(clouds, labels):
        store.add_frame(cloud)
        det.add_frame(store.size()[0] - 1, label)
        t0 = time.perf_counter()
        found += len(det.detect())
        spent += time.perf_counter() - t0
    small = ctx.get_profile()["small_launches"]
    det.close()
    store.close()
    return spent, found, small


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_ROOT, "profiles", "gicp", "timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--detect-rounds", type=int, default=5)
    args = ap.parse_args()

    _, labels, clouds = gr.l12_scans()
    s, t, start = gr.l12_pair(clouds, 6, 5)
    cases = [("l12_6_5", s, t, start)]
    for name, n in (("c3_20k", 20000), ("c3_100k", 100000)):
        src, tgt, _ = synth.c3_uniform(n, seed=61, perm_seed=62)
        cases.append((name, src, tgt, None))

    rule = (ref.EPSILON_DEFAULT, gr.L12_GATE)
    rule_small = rule + (True,)
    ctx = capi.Context(device=0, profile=1)
    out = {"gate_m": gr.L12_GATE, "epsilon": ref.EPSILON_DEFAULT, "iterations": args.iterations, "rounds": args.rounds,
           "cases": {}}
    for name, src, tgt, T0 in cases:
        cfg = capi.Context.make_config(args.iterations, 0.0, 0.0, T0)
        passes = args.iterations + 1

        def run(form):
            ctx.reset_profile()
            if form in ("gicp", "gicp_small"):
                res, _hist, info = ctx.align_gicp(src, tgt, cfg, rule_small if form == "gicp_small" else rule)
                pairs = int(info.pairs)
            else:
                res, _hist, pairs = ctx.align_gated(src, tgt, cfg, gr.L12_GATE)
            p = ctx.get_profile()
            assert res.history_len == passes, (name, form, res.history_len)
            return {"loop_us_per_pass": 1e3 * p["loop_ms"] / passes, "call_ms": p["total_ms"],
                    "fixed_ms": p["total_ms"] - p["loop_ms"], "normals_ms": p["normals_ms"], "pairs": pairs,
                    "small_launches": p["small_launches"], "final_error": res.final_error}

        forms = FORMS + (("gicp_small",) if name in SMALL_CASES else ())
        for form in forms:                                           # warm-up of every form
            run(form)
        samples = {form: [] for form in forms}
        for _ in range(args.rounds):                                 # alternating
            for form in forms:
                samples[form].append(run(form))

        def stat(key):
            return {form: {"median": statistics.median(x[key] for x in v), "min": min(x[key] for x in v),
                           "max": max(x[key] for x in v)} for form, v in samples.items()}

        loop, fixed = stat("loop_us_per_pass"), stat("fixed_ms")
        out["cases"][name] = {"rows": [int(src.shape[0]), int(tgt.shape[0])], "loop_us_per_pass": loop, "fixed_ms": fixed,
                              "gicp_over_gated": loop["gicp"]["median"] / loop["gated"]["median"], "samples": samples}
        print("%-8s %7d -> %7d rows: gated %9.2f us per pass (%.2f..%.2f), plane-to-plane %9.2f (%.2f..%.2f), x %.3f; fixed part "
              "%.3f ms against %.3f ms; pairs %d / %d; small kernel %s / %s"
              % (name, src.shape[0], tgt.shape[0], loop["gated"]["median"], loop["gated"]["min"], loop["gated"]["max"],
                 loop["gicp"]["median"], loop["gicp"]["min"], loop["gicp"]["max"], out["cases"][name]["gicp_over_gated"],
                 fixed["gated"]["median"], fixed["gicp"]["median"], samples["gated"][0]["pairs"], samples["gicp"][0]["pairs"],
                 samples["gated"][0]["small_launches"] > 0, samples["gicp"][0]["small_launches"] > 0))
        if "gicp_small" in samples:
            assert samples["gicp_small"][0]["small_launches"] > 0 and samples["gicp"][0]["small_launches"] == 0
            out["cases"][name]["small_over_gated"] = loop["gicp_small"]["median"] / loop["gated"]["median"]
            out["cases"][name]["small_over_general"] = loop["gicp_small"]["median"] / loop["gicp"]["median"]
            print("%-8s plane-to-plane, small form %9.2f us per pass (%.2f..%.2f): x %.3f of the gated kernel, x %.3f of the "
                  "general path; fixed part %.3f ms; pairs %d"
                  % (name, loop["gicp_small"]["median"], loop["gicp_small"]["min"], loop["gicp_small"]["max"],
                     out["cases"][name]["small_over_gated"], out["cases"][name]["small_over_general"],
                     fixed["gicp_small"]["median"], samples["gicp_small"][0]["pairs"]))

    # the whole detect() on L12, wall time
    for mode in DETECT_MODES:                                        # warm-up: the helper contexts and their workspaces
        detect_wall(ctx, clouds, labels, mode)
    walls = {mode: [] for mode in DETECT_MODES}
    for _ in range(args.detect_rounds):
        for mode in DETECT_MODES:
            spent, found, small = detect_wall(ctx, clouds, labels, mode)
            walls[mode].append({"detect_ms": 1e3 * spent, "closures": found, "small_launches": small})
    out["l12_detect"] = {"rounds": args.detect_rounds, "frames": len(clouds), "modes": {}}
    for mode, v in walls.items():
        ms = [x["detect_ms"] for x in v]
        out["l12_detect"]["modes"][mode] = {"detect_ms": {"median": statistics.median(ms), "min": min(ms), "max": max(ms)},
                                            "closures": v[0]["closures"], "small_launches": v[0]["small_launches"], "samples": v}
        print("L12 detect() %-6s %8.2f ms (%.2f..%.2f) over %d frames, %d closures, %d small-cloud launches"
              % (mode, statistics.median(ms), min(ms), max(ms), len(clouds), v[0]["closures"], v[0]["small_launches"]))
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
