"""scripts/gated_timing.py -- what the correspondence-distance gate costs per pass: device time of the
iteration loop (HIP events around it, icpmi_profile.loop_ms) of icpmi_align_gated against icpmi_align on the same pairs,

    l12_6_5       an L12 pair (4,342 -> 4,372 rows) from its verification's start: the small-cloud kernel, both
    c3_20k        20,000 -> 20,000 uniform points: past the small-cloud kernel; ungated the fused bounded loop, gated
                  search + k_reduce_gated + k_finish_step_gated + k_transform
    c3_100k       100,000 -> 100,000: ungated the culled engine

with tolerance 0 and min_error 0, so that both run exactly max_iterations passes and the post-loop one.  The two forms
alternate on one context, seven rounds after a warm-up of each; the medians and every sample go to
profiles/gated/timing.json.  Nothing is asserted.

    python scripts/gated_timing.py [--out profiles/gated/timing.json] [--rounds 7] [--iterations 20]"""
import argparse
import json
import os
import statistics
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: F401,E402  (first: one HIP runtime per process)

import gated_icp_ref as ref  # noqa: E402
from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_ROOT, "profiles", "gated", "timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=20)
    args = ap.parse_args()

    _, _, clouds = ref.l12_scans()
    s, t, start = ref.l12_pair(clouds, 6, 5)
    cases = [("l12_6_5", s, t, start)]
    for name, n in (("c3_20k", 20000), ("c3_100k", 100000)):
        src, tgt, _ = synth.c3_uniform(n, seed=61, perm_seed=62)
        cases.append((name, src, tgt, None))

    ctx = capi.Context(device=0, profile=1)
    out = {"gate_m": ref.L12_GATE, "iterations": args.iterations, "rounds": args.rounds, "cases": {}}
    for name, src, tgt, T0 in cases:
        cfg = capi.Context.make_config(args.iterations, 0.0, 0.0, T0)
        passes = args.iterations + 1

        def run(gated):
            ctx.reset_profile()
            if gated:
                res, _hist, pairs = ctx.align_gated(src, tgt, cfg, ref.L12_GATE)
            else:
                (res, _hist), pairs = ctx.align(src, tgt, cfg), src.shape[0]
            p = ctx.get_profile()
            assert res.history_len == passes, (name, gated, res.history_len)
            return {"loop_us_per_pass": 1e3 * p["loop_ms"] / passes, "call_ms": p["total_ms"], "pairs": pairs,
                    "small_launches": p["small_launches"], "final_error": res.final_error}

        run(False), run(True)                                        # warm-up of both forms
        samples = {"ungated": [], "gated": []}
        for _ in range(args.rounds):                                 # alternating
            samples["ungated"].append(run(False))
            samples["gated"].append(run(True))
        med = {k: statistics.median(x["loop_us_per_pass"] for x in v) for k, v in samples.items()}
        out["cases"][name] = {"rows": [int(src.shape[0]), int(tgt.shape[0])], "median_loop_us_per_pass": med,
                              "gated_over_ungated": med["gated"] / med["ungated"], "samples": samples}
        print("%-8s %7d -> %7d rows: ungated %9.2f us per pass, gated %9.2f (x %.2f), pairs %d, small kernel %s / %s"
              % (name, src.shape[0], tgt.shape[0], med["ungated"], med["gated"], med["gated"] / med["ungated"],
                 samples["gated"][0]["pairs"], samples["ungated"][0]["small_launches"] > 0,
                 samples["gated"][0]["small_launches"] > 0))
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
