"""scripts/robust_timing.py -- what robust row weights cost per pass: device time of the iteration loop
(HIP events around it, icpmi_profile.loop_ms) of icpmi_align_robust (Huber 0.1 m behind the 2 m gate) against
icpmi_align_gated at the same gate and icpmi_align on the same pairs,

    l12_6_5       an L12 pair (4,342 -> 4,372 rows) from its verification's start: the small-cloud kernel, all three
    c3_20k        20,000 -> 20,000 uniform points: past the small-cloud kernel; ungated the fused bounded loop, gated and
                  robust search + k_reduce_gated / k_reduce_robust + their step kernel + k_transform
    c3_100k       100,000 -> 100,000: ungated the culled engine

with tolerance 0 and min_error 0, so that all run exactly max_iterations passes and the post-loop one.  The three forms
alternate on one context, seven rounds after a warm-up of each; the medians and every sample go to
profiles/robust/timing.json.  The gated and ungated kernels are unchanged by the weights, so they are the baseline.
Nothing is asserted.

    python scripts/robust_timing.py [--out profiles/robust/timing.json] [--rounds 7] [--iterations 20]"""
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

import gated_icp_ref as gr  # noqa: E402
import robust_icp_ref as ref  # noqa: E402
from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402

FORMS = ("ungated", "gated", "robust")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(_ROOT, "profiles", "robust", "timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=20)
    args = ap.parse_args()

    _, _, clouds = gr.l12_scans()
    s, t, start = gr.l12_pair(clouds, 6, 5)
    cases = [("l12_6_5", s, t, start)]
    for name, n in (("c3_20k", 20000), ("c3_100k", 100000)):
        src, tgt, _ = synth.c3_uniform(n, seed=61, perm_seed=62)
        cases.append((name, src, tgt, None))

    rule = (capi.ROBUST_HUBER, ref.HUBER_SCALE, gr.L12_GATE)
    ctx = capi.Context(device=0, profile=1)
    out = {"gate_m": gr.L12_GATE, "kind": "huber", "scale_m": ref.HUBER_SCALE, "iterations": args.iterations,
           "rounds": args.rounds, "cases": {}}
    for name, src, tgt, T0 in cases:
        cfg = capi.Context.make_config(args.iterations, 0.0, 0.0, T0)
        passes = args.iterations + 1

        def run(form):
            ctx.reset_profile()
            weight_sum = None
            if form == "robust":
                res, _hist, info = ctx.align_robust(src, tgt, cfg, rule)
                pairs, weight_sum = int(info.pairs), float(info.weight_sum)
            elif form == "gated":
                res, _hist, pairs = ctx.align_gated(src, tgt, cfg, gr.L12_GATE)
            else:
                (res, _hist), pairs = ctx.align(src, tgt, cfg), src.shape[0]
            p = ctx.get_profile()
            assert res.history_len == passes, (name, form, res.history_len)
            return {"loop_us_per_pass": 1e3 * p["loop_ms"] / passes, "call_ms": p["total_ms"], "pairs": pairs,
                    "weight_sum": weight_sum, "small_launches": p["small_launches"], "final_error": res.final_error}

        for form in FORMS:                                           # warm-up of every form
            run(form)
        samples = {form: [] for form in FORMS}
        for _ in range(args.rounds):                                 # alternating
            for form in FORMS:
                samples[form].append(run(form))
        med = {k: statistics.median(x["loop_us_per_pass"] for x in v) for k, v in samples.items()}
        out["cases"][name] = {"rows": [int(src.shape[0]), int(tgt.shape[0])], "median_loop_us_per_pass": med,
                              "robust_over_gated": med["robust"] / med["gated"],
                              "robust_over_ungated": med["robust"] / med["ungated"], "samples": samples}
        print("%-8s %7d -> %7d rows: ungated %9.2f us per pass, gated %9.2f, robust %9.2f (x %.3f of gated), pairs %d, "
              "weight sum %.3f, small kernel %s / %s / %s"
              % (name, src.shape[0], tgt.shape[0], med["ungated"], med["gated"], med["robust"], med["robust"] / med["gated"],
                 samples["robust"][0]["pairs"], samples["robust"][0]["weight_sum"],
                 samples["ungated"][0]["small_launches"] > 0, samples["gated"][0]["small_launches"] > 0,
                 samples["robust"][0]["small_launches"] > 0))
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
