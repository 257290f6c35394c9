"""Culled full passes of the all-pairs engine (LoopPlan::cull_full in csrc/loop_plan.h, k_row_group_cull in nn_culled.h, the
loop of icpmi_align in capi.hip): a call's first two passes, which list every row, run k_nn_coarse_groups over
the (32-row tile, split) pairs that survive the box test instead of all pairs.  No result may change in any bit: every
case runs in child processes, one per setting of the knobs, with ICPMI_NN_CULL_FULL=0 (the launches of the form before) as
the reference leg, and pose, error history, final error, iteration count, flag, the matches the call leaves, the normal
matrix and the rows listed and certified per pass are compared byte for byte.

Shapes (the smallest that reach each form): 33,000 rows against 26,000 points (13 splits: the first size of the window;
k_nn_resolve_bounded with the match margin), 5,000 against 26,000 (k_nn_resolve4_bounded, list reuse without the margin),
66,000 against 40,000 (k_sum_groups, hence lean passes; also with ICPMI_NN_LEAN_FROM=3).  33,000 = 515 x 64 + 40 and
5,000 = 78 x 64 + 8: neither a multiple of 64 nor of 32; 33,013 besides.  Calls of k iterations on ONE context, k = 0, 1, 2,
3, 9, without a stopping test: the matches call k leaves are those of its pass k + 1, and every call meets what the call
before left in the per-row buffers and the group lists.

`passes` below is the number of passes the host queued (bounded_launches): nn_full_culled_passes, counted on the host like
it, must be min(2, passes) with the switch on and 0 with it off.
Marked gpu: runs on the MI355X box only."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch  # noqa: F401
from lidar_slam_from_scratch_amd import capi, dist as icpdist, synth

jobs = sys.argv[2].split(",")
hexes = lambda v: [float.hex(float(x)) for x in v]

def pair(n, m, seed=31):
    s, t, T = synth.c3_uniform(max(n, m), seed=seed, perm_seed=seed + 1)
    rng = np.random.Generator(np.random.PCG64(seed + 2))
    if n > s.shape[0]:   # further source rows: jittered copies of target points, moved like the others
        more = t[rng.integers(0, t.shape[0], n - s.shape[0])] + rng.normal(0.0, 0.01, size=(n - s.shape[0], 3))
        s = np.concatenate([s, synth.apply_transform(synth.invert_transform(T), more)])
    return np.ascontiguousarray(s[:n]), np.ascontiguousarray(t[:m])

def record(ctx, res, hist, n):
    idx, cur, perm, ok = ctx.debug_loop_rows(n)
    assert ok
    rows, blocks = ctx.nn_reuse_passes()
    p = ctx.get_profile()
    try:
        nm = ctx.last_normal_matrix()
        nmh = hexes(nm.JtJ.reshape(-1)) + hexes(nm.Jtb) + hexes([nm.sum_sq, nm.weight, nm.pairs]) + hexes(nm.T.reshape(-1))
    except capi.IcpError:
        nmh = None
    return {"T": hexes(res.transformation[:]), "hist": hexes(hist), "iters": int(res.num_iterations), "conv": int(res.converged),
            "final": float.hex(res.final_error), "idx": hashlib.sha256(idx.tobytes()).hexdigest(), "unmatched": int((idx < 0).sum()),
            "nm": nmh, "rows": [int(r) for r in rows], "cert": [int(c) for c in ctx.nn_margin_passes()],
            "full": int(p["nn_full_culled_passes"]), "passes": int(p["bounded_launches"]), "group_pairs": int(p["nn_group_pairs"]),
            "group_pairs_run": int(p["nn_group_pairs_run"]), "lean": int(p["nn_lean_passes"]), "n": int(n)}

def one(ctx, src, tgt, k, tol=0.0, min_error=0.0, T0=None):
    ctx.reset_profile()
    res, hist = ctx.align(src, tgt, capi.Context.make_config(max_iterations=k, tolerance=tol, min_error=min_error, initial_transform=T0))
    return record(ctx, res, hist, src.shape[0])

def new_ctx(search=capi.SEARCH_MFMA_BF16):
    return capi.Context(device=0, search=search, profile=1)

out = {}
for job in jobs:
    if job == "calls":     # shape A: calls of 0, 1, 2, 3 and 9 iterations on one context, the last once more
        src, tgt = pair(33000, 26000)
        ctx = new_ctx()
        out[job] = {str(k): one(ctx, src, tgt, k) for k in (0, 1, 2, 3, 9)}
        out[job]["again"] = one(ctx, src, tgt, 9)
        # ... then a smaller and a larger source on the same context (the group lists and per-row buffers are reused and regrown)
        out[job]["smaller"] = one(ctx, src[:20011], tgt, 3)
        big, _ = pair(41000, 26000)
        out[job]["larger"] = one(ctx, big, tgt, 3)
        out[job]["odd"] = one(ctx, big[:33013], tgt, 3)
        ctx.close()
    elif job == "stops":   # the stopping test ends the loop in pass 1 (min_error) and in pass 2 (tolerance)
        src, tgt = pair(33000, 26000)
        ctx = new_ctx()
        out[job] = {"pass1": one(ctx, src, tgt, 9, min_error=1e30), "pass2": one(ctx, src, tgt, 9, tol=1e30)}
        ctx.close()
    elif job == "edges":
        src, tgt = pair(33000, 26000)
        ctx = new_ctx()
        # the source starts 40 m beside the target's box (140 m along x): bounds that span the target, lists that overflow
        out["beside"] = {str(k): one(ctx, src, tgt, k, T0=synth.make_transform([0.0, 0.0, 0.0], [140.0, 0.0, 0.0])) for k in (1, 3)}
        # NaN rows sort to the front of the rows' Morton order and +Inf rows to its end: 70 NaN rows fill the first wave of
        # 64 rows (two whole tiles) and part of the next tile, 40 Inf rows fill the last wave's 40 rows (one whole tile and 8)
        s = src.copy()
        s[np.arange(70) * 471 + 5, 1] = np.nan
        s[np.arange(40) * 801 + 7, 2] = np.inf
        out["nonfinite"] = {str(k): one(ctx, s, tgt, k) for k in (0, 1, 3)}
        # ... and behind an initial transform that maps nothing to NaN but the rows themselves
        out["nonfinite"]["moved"] = one(ctx, s, tgt, 2, T0=synth.make_transform([0.0, 0.0, 0.01], [0.2, -0.1, 0.0]))
        # every target point twice: exact ties between two indices for every row
        t2 = np.ascontiguousarray(np.concatenate([tgt[:13000], tgt[:13000]]))
        out["ties"] = {str(k): one(ctx, src, t2, k) for k in (1, 3)}
        ctx.close()
    elif job == "shapes":  # shape B (k_nn_resolve4_bounded) and shape C (lean passes)
        src, tgt = pair(5000, 26000)
        ctx = new_ctx()
        out["b"] = {str(k): one(ctx, src, tgt, k) for k in (0, 1, 2, 9)}
        ctx.close()
        src, tgt = pair(66000, 40000)
        ctx = new_ctx()
        out["c"] = {str(k): one(ctx, src, tgt, k) for k in (1, 2, 12)}
        ctx.close()
    elif job == "elsewhere":   # where the plan keeps all pairs
        src, tgt = pair(33000, 26000)
        ctx = new_ctx()
        res, hist, kept = ctx.align_gated(src, tgt, capi.Context.make_config(max_iterations=3, tolerance=0.0, min_error=0.0), 2.0)
        p = ctx.get_profile()
        out["gated"] = {"full": int(p["nn_full_culled_passes"]), "hist": hexes(hist), "T": hexes(res.transformation[:])}
        out["splits10"] = one(ctx, src, np.ascontiguousarray(tgt[:20000]), 3)
        ctx.close()
        ctx = new_ctx(capi.SEARCH_MFMA_PRUNED)
        out["culled_engine"] = one(ctx, src, tgt, 3)
        ctx.close()
        group = icpdist.LocalGroup(2)
        def body(rank):
            lo, hi = icpdist.shard_bounds(src.shape[0], 2, rank)
            c = new_ctx()
            group.attach(c, rank)
            res, hist = c.align(src[lo:hi], tgt, capi.Context.make_config(max_iterations=3, tolerance=0.0, min_error=0.0))
            p = c.get_profile()
            c.comm_finalize(); c.close()
            return {"full": int(p["nn_full_culled_passes"]), "T": hexes(res.transformation[:]), "hist": hexes(hist)}
        out["sharded"] = group.run(body)
print(json.dumps(out))
"""

_LEGS = {}
_KNOBS = ("ICPMI_NN_CULL_FULL", "ICPMI_NN_REUSE", "ICPMI_NN_MARGIN", "ICPMI_NN_LEAN", "ICPMI_NN_LEAN_FROM", "ICPMI_FUSE_FINISH",
          "ICPMI_NN_BOUNDED", "ICPMI_KNN_CULL")


def _leg(jobs, **env_extra):
    """One child process: the jobs under one setting of the knobs.  Run once and shared by the tests below."""
    key = (jobs, tuple(sorted(env_extra.items())))
    if key not in _LEGS:
        env = dict(os.environ, ICPMI_SMALL="0", **env_extra)
        for k in _KNOBS:
            if k not in env_extra:
                env.pop(k, None)
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, jobs], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        _LEGS[key] = json.loads(r.stdout.strip().splitlines()[-1])
    return _LEGS[key]


RESULT = ("T", "hist", "iters", "conv", "final", "idx", "unmatched", "nm")


def _check(new, ref, what, counts=True):
    """One call, default against ICPMI_NN_CULL_FULL=0: every bit of the result, the rows listed and certified per pass, and
    the count of culled full passes."""
    bad = [k for k in RESULT if new[k] != ref[k]]
    assert not bad, (what, bad)
    if counts and (new["rows"] != ref["rows"] or new["cert"] != ref["cert"]):
        print(what, "rows listed  ", new["rows"], "\n   reference   ", ref["rows"], "\n   certified   ", new["cert"],
              "\n   reference   ", ref["cert"])
    if counts:
        assert new["rows"] == ref["rows"] and new["cert"] == ref["cert"], what
    assert new["passes"] == ref["passes"] and new["lean"] == ref["lean"], what
    assert new["full"] == min(2, new["passes"]) and ref["full"] == 0, (what, new["full"], new["passes"], ref["full"])
    # the culled engine's pair counters stay that engine's own
    assert new["group_pairs"] == 0 and new["group_pairs_run"] == 0, what


def test_calls_of_0_1_2_3_and_9_iterations():
    """33,000 -> 26,000: calls of 0, 1, 2, 3 and 9 iterations on one context (a call of 0 iterations has one pass, of one
    iteration two, the second its post-loop pass), and the last call once more."""
    new, ref = _leg("calls")["calls"], _leg("calls", ICPMI_NN_CULL_FULL="0")["calls"]
    for k in ("0", "1", "2", "3", "9", "again"):
        _check(new[k], ref[k], k)
    assert [new[k]["passes"] for k in ("0", "1", "2", "3", "9")] == [1, 2, 3, 4, 10]
    assert [new[k]["full"] for k in ("0", "1", "2", "3", "9")] == [1, 2, 2, 2, 2]
    assert new["9"]["rows"][0] == 33000 and new["9"]["unmatched"] == 0
    assert [new["again"][k] for k in RESULT] == [new["9"][k] for k in RESULT]


def test_smaller_larger_and_odd_sources_on_a_used_context():
    """... then 20,011, 41,000 and 33,013 rows on the same context: the lists of the call before are of another size."""
    new, ref = _leg("calls")["calls"], _leg("calls", ICPMI_NN_CULL_FULL="0")["calls"]
    for k, n in (("smaller", 20011), ("larger", 41000), ("odd", 33013)):
        _check(new[k], ref[k], k)
        assert new[k]["n"] == n and n % 32 and new[k]["full"] == 2


def test_stopping_test_in_pass_one_and_in_pass_two():
    """min_error above every error ends the loop in its first pass, a tolerance above every step in its second (the first
    iteration tests against DBL_MAX); the host has queued further passes by then, which do nothing."""
    new, ref = _leg("stops")["stops"], _leg("stops", ICPMI_NN_CULL_FULL="0")["stops"]
    assert (ref["pass1"]["iters"], ref["pass1"]["conv"]) == (1, 1) and (ref["pass2"]["iters"], ref["pass2"]["conv"]) == (2, 1)
    # (the rows listed per pass are read back for the passes queued: those behind the end did not run in either leg)
    _check(new["pass1"], ref["pass1"], "pass1")
    _check(new["pass2"], ref["pass2"], "pass2")


def test_far_start_nonfinite_rows_and_ties():
    """A start 40 m beside the target (bounds that span it, lists that overflow, the exhaustive search), rows with NaN and
    Inf coordinates that fill whole tiles and a whole wave of the sorted rows, and a target with every point twice."""
    new, ref = _leg("edges"), _leg("edges", ICPMI_NN_CULL_FULL="0")
    for name in ("beside", "nonfinite", "ties"):
        for k in ref[name]:
            _check(new[name][k], ref[name][k], (name, k))
    assert ref["beside"]["1"]["unmatched"] == 0
    assert ref["nonfinite"]["0"]["unmatched"] == 110   # a row with a non-finite coordinate has no neighbour
    assert ref["ties"]["3"]["unmatched"] == 0


def test_quarter_wave_resolve_and_lean_shapes():
    """5,000 -> 26,000 (k_nn_resolve4_bounded, no match margin) and 66,000 -> 40,000 (lean passes), the latter also with
    lean passes forced from the third pass on: the culled passes are the two in front of them."""
    new, ref = _leg("shapes"), _leg("shapes", ICPMI_NN_CULL_FULL="0")
    for name in ("b", "c"):
        for k in ref[name]:
            _check(new[name][k], ref[name][k], (name, k))
    assert new["b"]["9"]["cert"] == [] and new["c"]["12"]["cert"] != []
    forced, forced_ref = _leg("shapes", ICPMI_NN_LEAN_FROM="3")["c"], _leg("shapes", ICPMI_NN_LEAN_FROM="3", ICPMI_NN_CULL_FULL="0")["c"]
    for k in forced_ref:
        _check(forced[k], forced_ref[k], ("forced", k))
        assert [forced[k][f] for f in RESULT] == [ref["c"][k][f] for f in RESULT], k
    assert forced["12"]["lean"] == 11 and forced["12"]["full"] == 2


def test_all_pairs_everywhere_else():
    """No culled full pass without list reuse, under a gate, in the culled engine's own loop, in a two-rank sharded run and
    against a 20,000-point target (10 splits); and the same bits as with the switch off."""
    new, ref = _leg("elsewhere"), _leg("elsewhere", ICPMI_NN_CULL_FULL="0")
    assert new["gated"]["full"] == 0 and new["gated"] == ref["gated"]
    assert new["splits10"]["full"] == 0 and new["splits10"]["passes"] == 4 and new["splits10"] == ref["splits10"]
    assert new["culled_engine"]["full"] == 0 and new["culled_engine"]["group_pairs"] > 0 and new["culled_engine"] == ref["culled_engine"]
    assert [r["full"] for r in new["sharded"]] == [0, 0] and new["sharded"] == ref["sharded"]
    noreuse = _leg("calls", ICPMI_NN_REUSE="0")["calls"]
    on = _leg("calls")["calls"]
    for k in ("0", "1", "3", "9", "larger"):
        assert noreuse[k]["full"] == 0, k
        assert [noreuse[k][f] for f in ("T", "hist", "final", "idx")] == [on[k][f] for f in ("T", "hist", "final", "idx")], k
