#!/usr/bin/env python3
"""The stopping tests of the ICP loop (icp.hpp:210-217), fuzzed on the GPU against the oracle loop (run on the GPU box).

"Same iteration count" is the north_star's own gate, and it is decided by `error < min_error` and
`|prev_error - error| < tolerance` on an error whose last bits depend on the order of the additions.  Every trial is a
registration with the CALLER's settings (slam_node.cpp:134-138: 50 iterations, tolerance 1e-6, min_error 1e-9) on
well-conditioned geometry -- LiDAR-like frame pairs of the synthetic street at random frames, beam counts and voxel
sizes, and room corners (three planes) with random motions and noise -- through every MFMA engine (all pairs, culled,
AUTO) and held to ONE OF THE ORACLE'S TWO OUTCOMES: the oracle loop with its sums in index order (the index leg) and,
where that is needed, with every sum in reversed row order (the reversed leg, scripts/iteration_sensitivity.py).

The verdict on one engine run is `classify`, a pure function of three results (no GPU, no oracle call).  The OUTCOME of a
result is (num_iterations, converged, len(history)); its CALLER VIEW is what slam_node.cpp:139-140 makes of it: the
identity where `!converged || final_error > 1.0` (discarded), the pose otherwise (accepted), with final_error.

 1. outcome equal to the index leg's, which converged: pose within 1e-4 m / 1e-4 rad and history within 1e-9 (the
    north_star's tolerances) -> OK, anything else -> MISMATCH.  A settled loop has no excuse.
 2. outcome equal to the index leg's, which ran out of its iterations (frames three apart at 16 beams: error 0.58 and
    oscillating, kappa 1e6 -- every rounding difference is amplified step by step): inside the same tolerances -> OK;
    otherwise SENSITIVE only if pose, history and final_error are within eight times what the ORACLE ITSELF moves by
    between its two legs (+1e-12), the reversed leg has the same outcome, and every caller view is "discarded" (seed
    411087: the oracle moves 1.4e-4 m / 7.2e-5 rad / 1.4e-6 in the history, the GPU differs from it by 1.3e-4 / 6.7e-5 /
    3.6e-7); anything else -> MISMATCH.
 3. outcome different from the index leg's: MISMATCH if the two legs agree with each other, or if the engine's outcome is
    neither leg's (seed 320287: 28 iterations converged in index order, 50 unconverged reversed -- an engine returning 37
    is wrong there); SENSITIVE if it is the reversed leg's outcome AND the engine's caller view is that leg's (both
    discarded, or both accepted with poses within 1e-4 / 1e-4 and final_error within 1e-9); MISMATCH otherwise.
 4. a trial whose MARGIN is at or under 1e-12 (margin = the smallest distance of any stopping test the oracle evaluated
    from flipping, min over the loop's iterations of | |prev - err| - tolerance | and | err - min_error |, from the
    oracle's own history) is COUNTED and printed; a differing outcome is not held against the run there.

SENSITIVE is not a pass by itself: the seed has to be in PINNED_SENSITIVE below with the same kind (tests/
test_stopping_rule.py guards those seeds' generator and oracle side on the CPU, tests/test_gpu_stopping_pinned.py runs
them through the engines); any other is printed as UNPINNED SENSITIVE and fails the run until someone has looked at it.
The run also fails when the distinct sensitive seeds, or the under-margin trials, exceed trials // 100.
usage: python scripts/fuzz_stopping.py [trials] [first_seed]"""
import collections
import os
import sys
import time

import numpy as np
import torch  # noqa: F401
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402

MAX_IT, TOL, MIN_ERR = 50, 1e-6, 1e-9      # slam_node.cpp:134-138
MARGIN_FLOOR = 1e-12
POSE_TOL_M, POSE_TOL_RAD, HISTORY_TOL = 1e-4, 1e-4, 1e-9    # the north_star's tolerances
OWN_SPREAD_FACTOR, OWN_SPREAD_FLOOR = 8.0, 1e-12
GATE_MAX_ERROR = 1.0                       # slam_node.cpp:139-140: !converged || final_error > 1.0 -> identity

OK, SENSITIVE, MISMATCH = "OK", "SENSITIVE", "MISMATCH"
COUNT_MOVES, UNSETTLED = "count moves", "unsettled"
# The registrations that may be SENSITIVE, each looked at by hand.  "count moves": the oracle's own two
# legs leave the loop at different iterations; "unsettled": both legs run out of their 50 iterations and part on the way.
PINNED_SENSITIVE = {
    320287: COUNT_MOVES,   # lidar f124+2 b16 az900 v0.3: 28 converged in index order, 50 unconverged reversed
    411087: UNSETTLED,     # lidar f125+3 b16 az900 v0.5: the legs 1.4e-4 m / 7.2e-5 rad apart
    321727: UNSETTLED,     # lidar f124+1 b32 az1800 v0.3: 8.4e-11 m / 2.8e-12 rad
    321759: UNSETTLED,     # lidar f124+1 b16 az450 v0.3: 1.2e-5 m / 4.4e-7 rad
    91000: UNSETTLED,      # lidar f123+2 b16 az900 v0.8: 2.5e-13 m / 8e-15 rad
    320008: UNSETTLED,     # lidar f122+3 b16 az900 v0.5: 1.8e11 m / 1.66 rad
}

Run = collections.namedtuple("Run", "num_iterations converged history pose final_error")


def run_of_engine(res, hist):
    """an icpmi_result and the history icpmi_align filled -> Run"""
    return Run(int(res.num_iterations), bool(res.converged), np.array(hist, dtype=np.float64),
               np.array(res.transformation[:], dtype=np.float64).reshape(4, 4), float(res.final_error))


def run_of_oracle(ref):
    """oracle.icp_point_to_plane's result -> Run"""
    return Run(int(ref.num_iterations), bool(ref.converged), np.array(ref.error_history, dtype=np.float64),
               np.array(ref.transformation, dtype=np.float64).reshape(4, 4), float(ref.final_error))


def run_of_margins(r):
    """iteration_sensitivity.registration_margins' result -> Run (final_error is the post-loop entry, icp.hpp:251-252)"""
    return Run(int(r["num_iterations"]), bool(r["converged"]), np.array(r["history"], dtype=np.float64),
               np.array(r["transformation"], dtype=np.float64).reshape(4, 4), float(r["history"][-1]))


def outcome(run):
    return (run.num_iterations, run.converged, len(run.history))


def discarded(run):
    """slam_node.cpp:139-140: the caller replaces the pose by the identity"""
    return (not run.converged) or run.final_error > GATE_MAX_ERROR


def caller_view(run):
    return (np.eye(4) if discarded(run) else run.pose, run.final_error)


def deltas(a, b):
    """(pose m, pose rad, history, final_error) between two runs; the history's is inf where the lengths differ.  A NaN on
    either side gives NaN, which no `<=` below accepts."""
    dt, dr = synth.pose_delta(a.pose, b.pose)
    if not (np.isfinite(a.pose).all() and np.isfinite(b.pose).all()):
        dt = dr = float("nan")
    hd = float("inf")
    if len(a.history) == len(b.history) and len(a.history):
        both = np.isfinite(a.history).all() and np.isfinite(b.history).all()
        hd = float(np.abs(a.history - b.history).max()) if both else float("nan")
    return dt, dr, hd, abs(a.final_error - b.final_error)


def within_north_star(d):
    """(final_error is the history's last entry on every side, icp.hpp:251-252, so it is held like one)"""
    return bool(d[0] <= POSE_TOL_M and d[1] <= POSE_TOL_RAD and d[2] <= HISTORY_TOL and d[3] <= HISTORY_TOL)


def same_caller_view(a, b):
    if discarded(a) or discarded(b):
        return discarded(a) and discarded(b)
    d = deltas(a, b)
    return bool(d[0] <= POSE_TOL_M and d[1] <= POSE_TOL_RAD and d[3] <= HISTORY_TOL)


def needs_reversed(engine, leg_index):
    """Whether `classify` needs the reversed leg to judge this run (the second oracle run is made only then)."""
    if outcome(engine) != outcome(leg_index):
        return True
    return (not leg_index.converged) and not within_north_star(deltas(engine, leg_index))


def classify(engine, leg_index, leg_reversed=None):
    """The verdict on one engine run -> (OK | SENSITIVE | MISMATCH, reason); a SENSITIVE reason starts with its kind
    (COUNT_MOVES or UNSETTLED).  Pure: three Runs in, no GPU and no oracle call.  `leg_reversed` may be None where
    `needs_reversed` says so."""
    if needs_reversed(engine, leg_index) and leg_reversed is None:
        raise ValueError("this run cannot be judged without the oracle's reversed leg")
    d = deltas(engine, leg_index)
    what = "pose %.3g m %.3g rad, history %.3g, final_error %.3g against the index leg" % d
    if outcome(engine) == outcome(leg_index):
        if within_north_star(d):
            return OK, what
        if leg_index.converged:
            return MISMATCH, "a settled loop (%d iterations, converged): %s" % (leg_index.num_iterations, what)
        if outcome(leg_reversed) != outcome(leg_index):
            return MISMATCH, "an unsettled index leg %s whose reversed leg is %s: %s" % (outcome(leg_index), outcome(leg_reversed), what)
        if not (discarded(engine) and discarded(leg_index) and discarded(leg_reversed)):
            return MISMATCH, "an unsettled loop that the caller's gate does not discard on every side: %s" % what
        own = deltas(leg_index, leg_reversed)
        if all(x <= OWN_SPREAD_FACTOR * o + OWN_SPREAD_FLOOR for x, o in zip(d, own)):
            return SENSITIVE, ("%s: an unsettled loop (%d iterations, not converged); %s, and the oracle's own legs are %.3g m "
                               "%.3g rad %.3g %.3g apart" % ((UNSETTLED, leg_index.num_iterations, what) + own))
        return MISMATCH, ("an unsettled loop, more than %g times the oracle's own spread away: %s; the oracle's own legs are "
                          "%.3g m %.3g rad %.3g %.3g apart" % ((OWN_SPREAD_FACTOR, what) + own))
    counts = "outcome %s, the index leg's %s, the reversed leg's %s" % (outcome(engine), outcome(leg_index), outcome(leg_reversed))
    if outcome(leg_reversed) == outcome(leg_index):
        return MISMATCH, counts + ": the oracle's outcome does not move under reversed summation"
    if outcome(engine) != outcome(leg_reversed):
        return MISMATCH, counts + ": neither of the oracle's two"
    if not same_caller_view(engine, leg_reversed):
        return MISMATCH, counts + ": the reversed leg's, but not what the caller sees of it (%s against %s, %s)" % (
            "discarded" if discarded(engine) else "accepted", "discarded" if discarded(leg_reversed) else "accepted",
            "pose %.3g m %.3g rad, history %.3g, final_error %.3g" % deltas(engine, leg_reversed))
    return SENSITIVE, "%s: %s, the caller's view equal to the reversed leg's (%s)" % (
        COUNT_MOVES, counts, "discarded" if discarded(engine) else "accepted")


def make_case(seed):
    rng = np.random.default_rng(seed)
    if rng.random() < 0.6:
        # a frame pair of the synthetic street: frames a few steps apart, random resolution and voxel size
        f0 = int(rng.integers(0, 150))
        gap = int(rng.choice([1, 1, 2, 3]))
        beams = int(rng.choice([16, 32, 64]))
        az = int(rng.choice([450, 900, 1800]))
        voxel = float(rng.choice([0.3, 0.5, 0.8]))
        tgt = synth.lidar_frame(f0, voxel=voxel, beams=beams, azimuths=az)
        src = synth.lidar_frame(f0 + gap, voxel=voxel, beams=beams, azimuths=az)
        return src, tgt, "lidar f%d+%d b%d az%d v%.1f" % (f0, gap, beams, az, voxel)
    # a room corner: three orthogonal planes, source an independent noisy sample moved by a small rigid motion
    n_t = int(rng.choice([3000, 8000, 20000, 45000, 70000]))
    n_s = int(rng.choice([2000, 5000, 12000, 40000]))
    noise = float(rng.choice([0.002, 0.005, 0.02]))
    ext = float(rng.choice([10.0, 20.0, 40.0]))
    tgt = synth._room_corner(n_t, seed * 2 + 1, noise=noise, extent=ext)
    src0 = synth._room_corner(n_s, seed * 2 + 2, noise=noise, extent=ext)
    T = synth.make_transform(rng.normal(0, 0.015, 3), rng.normal(0, 0.08, 3))
    src = np.ascontiguousarray(synth.apply_transform(synth.invert_transform(T), src0))
    return src, tgt, "corner %d->%d noise %g ext %g" % (n_s, n_t, noise, ext)


def oracle_margin(ref):
    """Distance of the nearest evaluated stopping test from flipping, from the oracle's own history.  The history is
    e_0 .. e_k of the loop, then the post-loop entry (icp.hpp:235-252)."""
    h = np.asarray(ref.error_history, dtype=np.float64)
    loop = h[:-1]
    m = np.inf
    prev = np.finfo(np.float64).max
    for e in loop:
        m = min(m, abs(abs(prev - e) - TOL), abs(e - MIN_ERR))
        prev = e
    return float(m)


def _threads():
    return min(16, os.cpu_count() or 1)


def oracle_legs(src, tgt, which=("index", "reversed")):
    """The oracle loop restated on the oracle's primitives (iteration_sensitivity.registration_margins) with every sum in
    index order and in reversed row order -> a Run per entry of `which`."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import iteration_sensitivity as its
    return tuple(run_of_margins(its.registration_margins(src, tgt, MAX_IT, TOL, MIN_ERR, order=o, nthreads=_threads())) for o in which)


def record(stats, seed, verdict, reason):
    """One engine run's verdict into `stats` -> (1 if it counts as a mismatch, the label to print).  A SENSITIVE verdict on a
    seed that PINNED_SENSITIVE does not hold with that kind is UNPINNED: listed, and a failure in `failures`."""
    if verdict == OK:
        return 0, OK
    if verdict == MISMATCH:
        return 1, "MISMATCH stopping"
    stats["sensitive"] += 1
    stats["sensitive_seeds"].add(seed)
    kind = COUNT_MOVES if reason.startswith(COUNT_MOVES) else UNSETTLED
    if PINNED_SENSITIVE.get(seed) != kind:
        stats["unpinned"].add(seed)
        return 0, "UNPINNED SENSITIVE"
    return 0, SENSITIVE


def failures(stats, bad=0):
    """Why a run with these stopping-test statistics fails: a list of lines, empty where it passes.  The caps are counted on
    the stopping-test trials (`stats["trials"]`)."""
    cap = stats["trials"] // 100
    out = []
    if bad:
        out.append("%d mismatches" % bad)
    if stats["unpinned"]:
        out.append("sensitive seeds outside PINNED_SENSITIVE (or pinned as the other kind): %s" % sorted(stats["unpinned"]))
    if len(stats["sensitive_seeds"]) > cap:
        out.append("%d distinct sensitive seeds %s in %d trials, more than trials // 100 = %d"
                   % (len(stats["sensitive_seeds"]), sorted(stats["sensitive_seeds"]), stats["trials"], cap))
    if stats["under"] > cap:
        out.append("%d trials under the %g margin floor in %d trials, more than trials // 100 = %d"
                   % (stats["under"], MARGIN_FLOOR, stats["trials"], cap))
    return out


def summary(stats):
    return ("%d trials decided (smallest margin %.3g), %d under the 1e-12 floor, %d ran out of iterations in the oracle, %d engine "
            "runs SENSITIVE on %d distinct seeds %s, %d of them unpinned %s; cap on sensitive seeds and on under-margin trials %d"
            % (stats["decided"], stats["min_margin"], stats["under"], stats["exhausted"], stats["sensitive"],
               len(stats["sensitive_seeds"]), sorted(stats["sensitive_seeds"]), len(stats["unpinned"]), sorted(stats["unpinned"]),
               stats["trials"] // 100))


def check_case(seed, ctxs, cfg, stats):
    """One trial through every context of `ctxs` -> mismatches; `stats` (new_stats) is updated."""
    src, tgt, what = make_case(seed)
    ref = orc.icp_point_to_plane(src, tgt, MAX_IT, TOL, MIN_ERR, nthreads=_threads())
    margin = oracle_margin(ref)
    index = run_of_oracle(ref)      # (the restatement's index leg IS this loop, bit for bit: tests/test_stopping_rule.py)
    reversed_leg = None
    bad = 0
    stats["trials"] += 1
    if not ref.converged:
        stats["exhausted"] += 1
    if margin <= MARGIN_FLOOR:
        stats["under"] += 1
        print("UNDER MARGIN seed %d (%s): margin %.3g -- a differing outcome below is not held against the run" % (seed, what, margin))
    else:
        stats["decided"] += 1
        stats["min_margin"] = min(stats["min_margin"], margin)
    for name, ctx in ctxs.items():
        res, hist = ctx.align(src, tgt, cfg)
        engine = run_of_engine(res, hist)
        if margin <= MARGIN_FLOOR and outcome(engine) != outcome(index):
            print("NOT HELD seed %d (%s) engine %s: outcome %s against %s under the margin floor" % (seed, what, name, outcome(engine), outcome(index)))
            continue
        if reversed_leg is None and needs_reversed(engine, index):
            # The margin above is the distance of the ORACLE's stopping tests from flipping along the oracle's own
            # trajectory; it says nothing about a trajectory that is itself unstable.  So the oracle loop is run once more
            # with every sum in reversed row order, and the engine is held to one of the two.
            reversed_leg, = oracle_legs(src, tgt, ("reversed",))
            print("LEGS seed %d (%s): index %s final_error %r, reversed %s final_error %r"
                  % (seed, what, outcome(index), index.final_error, outcome(reversed_leg), reversed_leg.final_error))
        verdict, reason = classify(engine, index, reversed_leg)
        n, label = record(stats, seed, verdict, reason)
        bad += n
        if label != OK:
            print("%s seed %d (%s) engine %s: %s, margin %.3g" % (label, seed, what, name, reason, margin))
    return bad


def new_stats():
    return {"trials": 0, "decided": 0, "under": 0, "exhausted": 0, "min_margin": np.inf, "sensitive": 0, "sensitive_seeds": set(),
            "unpinned": set()}


def caller_config():
    return capi.Context.make_config(max_iterations=MAX_IT, tolerance=TOL, min_error=MIN_ERR)


def run_trials(seeds, ctxs, cfg, check=None):
    """`check_case` over `seeds` -> (exit code, mismatches, stats): the bookkeeping of `main` (tests stub `check`)."""
    check = check_case if check is None else check
    bad, stats = 0, new_stats()
    t0 = time.time()
    for t, seed in enumerate(seeds):
        bad += check(seed, ctxs, cfg, stats)
        if (t + 1) % 10 == 0:
            print("%d trials, %d mismatches, %d under the margin floor, %d sensitive seeds, %.0f s"
                  % (t + 1, bad, stats["under"], len(stats["sensitive_seeds"]), time.time() - t0), flush=True)
    why = failures(stats, bad)
    for line in why:
        print("FAIL fuzz_stopping: " + line)
    print("fuzz_stopping: %d trials x %d engines, %d mismatches; %s" % (stats["trials"], len(ctxs), bad, summary(stats)))
    return (1 if why else 0), bad, stats


def main(argv=None):
    argv = sys.argv if argv is None else argv
    trials = int(argv[1]) if len(argv) > 1 else 40
    seed0 = int(argv[2]) if len(argv) > 2 else 9000
    engines = {"auto": capi.SEARCH_AUTO, "all pairs": capi.SEARCH_MFMA_BF16, "culled": capi.SEARCH_MFMA_PRUNED}
    ctxs = {k: capi.Context(device=0, search=v) for k, v in engines.items()}
    try:
        return run_trials(range(seed0, seed0 + trials), ctxs, caller_config())[0]
    finally:
        for c in ctxs.values():
            c.close()


if __name__ == "__main__":
    sys.exit(main())
