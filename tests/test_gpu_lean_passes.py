"""Lean passes of the all-pairs engine (list_reuse.h "lean passes", WantPublish / k_sum_groups in kernels.h, the loop of
icpmi_align in capi.hip): once the passes the host knows of have listed no row, k_row_list and the coarse
kernel are no longer launched, and a row that does want a list takes the resolve's exhaustive search.  No result may
change in any bit: every case runs in child processes, one per setting of the knobs, with ICPMI_NN_LEAN=0 (the launches
of the form before) as the reference leg, and pose, error history, iteration count, flag, final error and the matches of
every pass are compared byte for byte.

The cloud: 66,000 source rows (1,032 partial rows: the smallest sizes that launch k_sum_groups start at 65,473) against
a 40,000-point target, whose 20 splits keep the rows in Morton order.  `per_pass` jobs run with max_iterations = 1 .. K on
ONE context and no stopping test: the matches the loop leaves after call k are those of pass k + 1 (the post-loop pass),
and every call meets what the call before left in the per-row buffers and in the host-mapped rings.

Where the stopping test ends a loop: the tolerances are taken from the reference history itself (bit-equal in every leg),
between a record-low step of the error and the smallest step before it, so the iteration the loop ends in is known.
Under the rule lean passes start four passes after the last row was listed, when the error's steps have long reached
rounding noise and no tolerance can place the end a priori; so the end INSIDE lean mode is placed with
ICPMI_NN_LEAN_FROM=5 (lean from the fifth pass on) and an end in iteration 7 or later, and a third leg runs the rule with
the smallest positive tolerance, wherever that ends.
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
tols = json.loads(sys.argv[3]) if len(sys.argv) > 3 else {}

def cloud(n_src, seed):
    # the C3-like pair at 40,000 points, and further source rows: jittered copies of target points, moved like the others
    s, t, T = synth.c3_uniform(40000, seed=seed, perm_seed=seed + 1)
    rng = np.random.Generator(np.random.PCG64(seed + 2))
    if n_src > s.shape[0]:
        more = t[rng.integers(0, t.shape[0], n_src - s.shape[0])] + rng.normal(0.0, 0.01, size=(n_src - s.shape[0], 3))
        s = np.concatenate([s, synth.apply_transform(synth.invert_transform(T), more)])
    return np.ascontiguousarray(s[:n_src]), t

def lattice(shape, step, seed):
    g = np.stack(np.meshgrid(*[np.arange(k, dtype=np.float64) * step for k in shape], indexing="ij"), -1).reshape(-1, 3)
    return g[np.random.default_rng(seed).permutation(g.shape[0])]

hexes = lambda v: [float.hex(float(x)) for x in v]
COUNTERS = ("nn_lean_passes", "nn_fallback_queries", "bounded_launches", "nn_launches", "reduce_launches",
            "transform_launches", "nn_coarse_blocks", "nn_coarse_skipped", "nn_rows_listed", "nn_rows_certified")

def one(ctx, src, tgt, k, tol=0.0, T0=None):
    ctx.reset_profile()
    res, hist = ctx.align(src, tgt, capi.Context.make_config(max_iterations=k, tolerance=tol, min_error=0.0, initial_transform=T0))
    idx, cur, perm, ok = ctx.debug_loop_rows(src.shape[0])
    assert ok
    rows, blocks = ctx.nn_reuse_passes()
    p = ctx.get_profile()
    return {"T": hexes(res.transformation[:]), "hist": hexes(hist), "iters": int(res.num_iterations), "conv": int(res.converged),
            "final": float.hex(res.final_error), "idx": hashlib.sha256(idx.tobytes()).hexdigest(), "unmatched": int((idx < 0).sum()),
            "rows": [int(r) for r in rows], "blocks": [int(b) for b in blocks], "cert": [int(c) for c in ctx.nn_margin_passes()],
            "prof": {c: int(p[c]) for c in COUNTERS}}

out = {}
src, tgt = cloud(66000, 21)
for job in jobs:
    if job == "per_pass24" or job == "per_pass10":   # per_pass10: profile level 2, where the resolve counts its exhaustive searches
        K = int(job[8:])
        ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=2 if K == 10 else 1)
        out[job] = {str(k): one(ctx, src, tgt, k) for k in range(1, K + 1)}
        out[job]["again"] = one(ctx, src, tgt, K)      # the last call once more: two calls on one context
        ctx.close()
    elif job == "tol":
        ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
        out[job] = {name: one(ctx, src, tgt, 24, tol=float.fromhex(t)) for name, t in tols.items()}
        ctx.close()
    elif job == "edge":
        ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
        # exact ties: a lattice target and the same lattice shifted by half a step in x and y (every row equidistant from four)
        t = lattice((40, 40, 42), 1.0, 27)
        s = t + np.array([0.5, 0.5, 0.0])
        T0 = synth.make_transform([0.0, 0.0, 0.002], [0.01, 0.0, 0.0])
        out["ties"] = {str(k): one(ctx, s, t, k, T0=T0) for k in (6, 12)}
        # a source with one NaN and one Inf row
        s = src.copy(); s[1234, 1] = np.nan; s[60001, 2] = np.inf
        out["nonfinite"] = {str(k): one(ctx, s, tgt, k) for k in (1, 10)}
        ctx.close()
    elif job == "small":   # a 40,000-row source: no k_sum_groups launch, hence no lean pass
        ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
        out[job] = one(ctx, src[:40000], tgt, 24)
        ctx.close()
    elif job == "fused24":  # the 24-iteration call alone (the ICPMI_FUSE_FINISH=0 legs)
        ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
        out[job] = one(ctx, src, tgt, 24)
        ctx.close()
    elif job == "sharded":  # two ranks (threads of this process) of 66,000 rows each: every rank launches k_sum_groups
        big, _ = cloud(132000, 21)
        group = icpdist.LocalGroup(2)
        def body(rank):
            lo, hi = icpdist.shard_bounds(big.shape[0], 2, rank)
            c = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
            group.attach(c, rank)
            res, hist = c.align(big[lo:hi], tgt, capi.Context.make_config(max_iterations=16, tolerance=0.0, min_error=0.0))
            rows, blocks = c.nn_reuse_passes()
            p = c.get_profile()
            c.comm_finalize(); c.close()
            return {"n": hi - lo, "T": hexes(res.transformation[:]), "hist": hexes(hist), "rows": [int(r) for r in rows],
                    "blocks": [int(b) for b in blocks], "prof": {c_: int(p[c_]) for c_ in COUNTERS}}
        out[job] = group.run(body)
print(json.dumps(out))
"""

_LEGS = {}


def _leg(jobs, tols=None, **env_extra):
    """One child process: the jobs under one setting of the knobs.  Run once and shared by the tests below."""
    key = (jobs, json.dumps(tols, sort_keys=True), tuple(sorted(env_extra.items())))
    if key not in _LEGS:
        env = dict(os.environ, ICPMI_SMALL="0", **env_extra)
        for k in ("ICPMI_NN_REUSE", "ICPMI_NN_MARGIN", "ICPMI_NN_LEAN", "ICPMI_NN_LEAN_FROM", "ICPMI_FUSE_FINISH"):
            if k not in env_extra:
                env.pop(k, None)
        args = [sys.executable, "-c", _CHILD, ROOT, jobs] + ([json.dumps(tols)] if tols else [])
        r = subprocess.run(args, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        _LEGS[key] = json.loads(r.stdout.strip().splitlines()[-1])
    return _LEGS[key]


RESULT = ("T", "hist", "iters", "conv", "final", "idx")


def _same_results(a, b, keys=RESULT):
    return [k for k in keys if a[k] != b[k]]


def _rule(rows):
    """The lean passes (from 1) the rule gives for the rows listed per pass."""
    return [p for p in range(7, len(rows) + 1) if rows[p - 5] == 0 and rows[p - 4] == 0]


def _default():
    return _leg("per_pass24,edge,small,sharded")


def _reference():
    return _leg("per_pass24,per_pass10,edge,small,sharded", ICPMI_NN_LEAN="0")


def _forced():
    return _leg("per_pass10,edge", ICPMI_NN_LEAN_FROM="3")


def test_lean_passes_change_no_bit():
    """Case 1: the default against ICPMI_NN_LEAN=0 over 24 iterations -- results, the matches of every pass, and the rows
    listed and certified per pass; lean passes did run, and they are the passes the rule gives for the rows listed."""
    new, ref = _default()["per_pass24"], _reference()["per_pass24"]
    for k in list(range(1, 25)):
        bad = _same_results(new[str(k)], ref[str(k)], RESULT + ("rows", "blocks", "cert", "unmatched"))
        assert not bad, (k, bad)
        assert ref[str(k)]["prof"]["nn_lean_passes"] == 0 and new[str(k)]["unmatched"] == 0
    last = new["24"]
    print("rows listed", last["rows"], "certified", last["cert"], "lean passes", last["prof"]["nn_lean_passes"])
    assert len(last["rows"]) == 25 and last["rows"][0] == last["rows"][1] == 66000
    assert last["prof"]["nn_lean_passes"] > 0
    for k in range(1, 25):   # a call of k iterations has k + 1 passes
        assert new[str(k)]["prof"]["nn_lean_passes"] == len(_rule(last["rows"][:k + 1])), k
    # a lean pass has no coarse launch, and nothing else about the launches differs
    # (nn_coarse_blocks: the coarse workgroups launched, the same number in each of the reference's 25 passes)
    lean = last["prof"]["nn_lean_passes"]
    assert ref["24"]["prof"]["nn_coarse_blocks"] % 25 == 0
    assert last["prof"]["nn_coarse_blocks"] == ref["24"]["prof"]["nn_coarse_blocks"] // 25 * (25 - lean)
    for c in ("bounded_launches", "nn_launches", "reduce_launches", "transform_launches", "nn_coarse_skipped", "nn_rows_listed",
              "nn_rows_certified"):
        assert last["prof"][c] == ref["24"]["prof"][c], c


def test_forced_lean_passes_answer_by_the_exhaustive_search():
    """Case 2: ICPMI_NN_LEAN_FROM=3 against ICPMI_NN_LEAN=0 over 10 iterations: rows that want a list get none from the third
    pass on, the resolve's exhaustive search answers them (nn_fallback_queries, counted at profile level 2), and no bit moves."""
    new, ref = _forced()["per_pass10"], _reference()["per_pass10"]
    for k in range(1, 11):
        bad = _same_results(new[str(k)], ref[str(k)])
        assert not bad, (k, bad)
        assert new[str(k)]["prof"]["nn_lean_passes"] == max(0, k + 1 - 2), k
    print("exhaustive searches, forced", new["10"]["prof"]["nn_fallback_queries"], "reference", ref["10"]["prof"]["nn_fallback_queries"],
          "rows wanted per pass", new["10"]["rows"])
    assert new["10"]["prof"]["nn_fallback_queries"] > ref["10"]["prof"]["nn_fallback_queries"] >= 0
    assert new["10"]["prof"]["nn_fallback_queries"] > 0
    assert sum(new["10"]["rows"][2:]) > 0   # rows did want lists in lean passes


def _tolerances():
    """From the reference history (24 iterations, no stopping test): step[k] = |hist[k] - hist[k + 1]| is what iteration
    k + 2 tests (the first iteration tests against DBL_MAX).  A tolerance between a record-low step and the smallest step
    before it -- for step[0], above it -- ends the loop in that step's iteration."""
    hist = [float.fromhex(h) for h in _reference()["per_pass24"]["24"]["hist"]]
    step = [abs(hist[k] - hist[k + 1]) for k in range(24)]
    record = [k for k in range(24) if k == 0 or step[k] < min(step[:k])]
    early = [k for k in record if k + 2 <= 5]
    late = [k for k in record if k + 2 >= 7]
    assert early and late, (record, step)

    def tol(k):
        if k == 0:
            return 2.0 * step[0]
        return min(step[:k]) if step[k] == 0.0 else (step[k] * min(step[:k])) ** 0.5
    return {"early": (early[-1] + 2, tol(early[-1])), "late": (late[0] + 2, tol(late[0]))}


def test_stopping_test_before_and_inside_lean_mode():
    """Case 3: a tolerance that ends the loop before any pass can be lean (iteration 5 at the latest), under the rule; one
    that ends it in iteration 7 or later with lean passes from the fifth on (ICPMI_NN_LEAN_FROM=5; see the module's
    docstring); and the smallest positive tolerance under the rule.  Every leg against ICPMI_NN_LEAN=0."""
    t = _tolerances()
    tols = {"early": float.hex(t["early"][1]), "late": float.hex(t["late"][1]), "tiny": float.hex(5e-324)}
    ref = _leg("tol", tols, ICPMI_NN_LEAN="0")["tol"]
    new = _leg("tol", tols)["tol"]
    forced = _leg("tol", tols, ICPMI_NN_LEAN_FROM="5")["tol"]
    for name, (it, _) in t.items():
        assert ref[name]["conv"] == 1 and ref[name]["iters"] == it, (name, it, ref[name]["iters"])
    print("ends in iterations", {k: v["iters"] for k, v in ref.items()}, "lean passes, rule", {k: v["prof"]["nn_lean_passes"] for k, v in new.items()},
          "forced", {k: v["prof"]["nn_lean_passes"] for k, v in forced.items()})
    for name in tols:
        assert not _same_results(new[name], ref[name]), name
        assert not _same_results(forced[name], ref[name]), name
    assert new["early"]["prof"]["nn_lean_passes"] == 0
    assert forced["late"]["prof"]["nn_lean_passes"] > 0   # the loop ended inside lean mode


def test_short_calls_and_ring_edges():
    """Case 4: max_iterations of 1, 2, 3 and 9 (the rings have 8 slots), under the rule and with lean passes forced from the
    third pass on; the host reads a count from the third iteration on."""
    ref = _reference()
    for k in ("1", "2", "3", "9"):
        assert not _same_results(_default()["per_pass24"][k], ref["per_pass24"][k]), k
        assert not _same_results(_forced()["per_pass10"][k], ref["per_pass10"][k]), k
        assert _default()["per_pass24"][k]["iters"] == int(k)


def test_two_calls_on_one_context():
    """Case 5: the same call twice on one context gives the same bits and the same lean passes, in every leg."""
    for leg, job, k in ((_default(), "per_pass24", "24"), (_reference(), "per_pass24", "24"), (_forced(), "per_pass10", "10")):
        a, b = leg[job][k], leg[job]["again"]
        assert not _same_results(a, b, RESULT + ("rows", "blocks", "cert")), job
        assert a["prof"]["nn_lean_passes"] == b["prof"]["nn_lean_passes"]
    assert not _same_results(_default()["per_pass24"]["again"], _reference()["per_pass24"]["again"])


def test_ties_and_nonfinite_rows():
    """Case 6: exact ties (never certified: the exhaustive search must break them as the listed path does) and a source
    with a NaN and an Inf row (no match in the first pass, a NaN pose from the first step on), under the rule and with
    lean passes forced from the third pass on."""
    ref = _reference()
    for leg in (_default(), _forced()):
        for name in ("ties", "nonfinite"):
            for k in ref[name]:
                assert not _same_results(leg[name][k], ref[name][k], RESULT + ("unmatched",)), (name, k)
    assert _forced()["ties"]["12"]["prof"]["nn_lean_passes"] == 11 and ref["ties"]["12"]["unmatched"] == 0
    assert ref["nonfinite"]["1"]["unmatched"] == 66000


def test_lean_passes_stay_off_elsewhere():
    """Case 7: ICPMI_FUSE_FINISH=0, a two-rank sharded run and a 40,000-row source: no lean pass, the launch counts of
    ICPMI_NN_LEAN=0, and the same bits."""
    new, ref = _default(), _reference()
    assert new["small"]["prof"]["nn_lean_passes"] == 0
    assert not _same_results(new["small"], ref["small"], RESULT + ("rows", "blocks", "cert", "prof"))
    for a, b in zip(new["sharded"], ref["sharded"]):
        assert a["prof"]["nn_lean_passes"] == 0 and a["n"] == 66000
        assert a == b
    assert new["sharded"][0]["T"] == new["sharded"][1]["T"] and new["sharded"][0]["hist"] == new["sharded"][1]["hist"]
    unf = _leg("fused24", ICPMI_FUSE_FINISH="0")["fused24"]
    unf_ref = _leg("fused24", ICPMI_FUSE_FINISH="0", ICPMI_NN_LEAN="0")["fused24"]
    assert unf["prof"]["nn_lean_passes"] == 0
    assert not _same_results(unf, unf_ref, RESULT + ("rows", "blocks", "cert", "prof"))
    assert not _same_results(unf, new["per_pass24"]["24"], RESULT + ("rows", "cert"))
