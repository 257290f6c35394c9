"""Solo passes of the all-pairs engine (csrc/solo_pass.h: k_finish_step_transform_solo; LoopPlan::solo_on and solo_next in
loop_plan.h; the loop of icpmi_align in capi.hip): once the passes the host knows of found every row
certified, the kernel that ends a pass also forms the next pass's terms and group sums, and that pass launches nothing
but its own tail.  No result may change in any bit: every case runs in child processes, one per setting of the knobs, with
ICPMI_NN_SOLO=0 (the three launches of the form before) as the reference leg, and pose, error history, iteration count,
flag, final error, the normal matrix of icpmi_last_normal_matrix, the matches of every pass, the rows listed and
certified per pass and the lean passes are compared byte for byte.

The clouds are the lean tests': cloud(n, 21) against its 40,000-point target, at the sizes on both sides of the plan's
window (65,472 | 65,473 ... 131,072 | 131,073 rows) and 66,000, whose last group sum has 8 members.  `per_pass` jobs run
with max_iterations = 1 .. K on ONE context and no stopping test: the matches the loop leaves after call k are those of
pass k + 1, and every call meets what the call before left in the buffers and in the host-mapped rings.  On these clouds
every row is certified from pass 8 on, so under the rule the tail of pass 11 is the first solo kernel.  The solo kernel's
own exhaustive search is reached with ICPMI_NN_SOLO_FROM=3 (tens of thousands of rows are not certified in passes 4-7):
results and the matches of every pass are the reference's; the per-pass statistics are not compared in that leg, since a
row searched there leaves no margin and is certified later than in the reference.  The same holds under the rule: were a
pass queued solo although a row of it is not certified, that row's later certificates -- not its matches -- would differ,
and the legs that compare `rows` and `cert` would report it as a statistics mismatch with equal results; on these clouds
the solo kernels search no row under the rule (nn_solo_fallback_rows == 0 is asserted).
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
from lidar_slam_from_scratch_amd import capi, synth

jobs = sys.argv[2].split(",")
tols = json.loads(sys.argv[3]) if len(sys.argv) > 3 else {}

def cloud(n_src, seed):
    # (the lean tests' construction) the C3-like pair at 40,000 points, and further source rows: jittered copies of target points
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
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
COUNTERS = ("nn_solo_passes", "nn_solo_fallback_rows", "nn_lean_passes", "bounded_launches", "nn_coarse_blocks", "nn_coarse_skipped",
            "nn_rows_listed", "nn_rows_certified")

def one(ctx, src, tgt, k, tol=0.0, T0=None):
    ctx.reset_profile()
    res, hist = ctx.align(src, tgt, capi.Context.make_config(max_iterations=k, tolerance=tol, min_error=0.0, initial_transform=T0))
    idx, cur, perm, ok = ctx.debug_loop_rows(src.shape[0])
    assert ok
    nm = ctx.last_normal_matrix()
    rows, blocks = ctx.nn_reuse_passes()
    p = ctx.get_profile()
    return {"T": hexes(res.transformation[:]), "hist": hexes(hist), "iters": int(res.num_iterations), "conv": int(res.converged),
            "final": float.hex(res.final_error), "idx": sha(idx), "cur": sha(cur), "unmatched": int((idx < 0).sum()),
            "nm": sha(np.concatenate([nm.JtJ.ravel(), nm.Jtb, [nm.sum_sq, nm.weight], nm.T.ravel()])),
            "rows": [int(r) for r in rows], "blocks": [int(b) for b in blocks], "cert": [int(c) for c in ctx.nn_margin_passes()],
            "prof": {c: int(p[c]) for c in COUNTERS}, "n": int(src.shape[0])}

out = {}
big, tgt = cloud(131073, 21)
for job in jobs:
    if job.startswith("per_pass"):      # per_pass16 / per_pass10: calls of 1 .. K iterations at 66,000 rows, the last one twice
        K = int(job[8:])
        ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
        out[job] = {str(k): one(ctx, big[:66000], tgt, k) for k in range(1, K + 1)}
        out[job]["again"] = one(ctx, big[:66000], tgt, K)
        ctx.close()
    elif job.startswith("size"):        # size65473: calls of 1, 2, 3, 9 and 16 iterations at that many rows, the last one twice
        n = int(job[4:])
        ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
        out[job] = {str(k): one(ctx, big[:n], tgt, k) for k in (1, 2, 3, 9, 16)}
        out[job]["again"] = one(ctx, big[:n], tgt, 16)
        ctx.close()
    elif job == "tol":
        ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
        out[job] = {name: one(ctx, big[:66000], tgt, 24, tol=float.fromhex(t)) for name, t in tols.items()}
        ctx.close()
    elif job == "edge":
        ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
        # exact ties: a lattice target and the same lattice shifted by half a step in x and y (every row equidistant from four)
        t = lattice((40, 40, 42), 1.0, 27)
        s = t + np.array([0.5, 0.5, 0.0])
        T0 = synth.make_transform([0.0, 0.0, 0.002], [0.01, 0.0, 0.0])
        out["ties"] = {str(k): one(ctx, s, t, k, T0=T0) for k in (6, 12)}
        # a source with one NaN and one Inf row
        s = big[:66000].copy(); s[1234, 1] = np.nan; s[60001, 2] = np.inf
        out["nonfinite"] = {str(k): one(ctx, s, tgt, k) for k in (1, 10)}
        ctx.close()
    elif job == "once16":               # the 16-iteration call at 66,000 rows alone (the legs with another knob off)
        ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
        out[job] = one(ctx, big[:66000], tgt, 16)
        ctx.close()
    elif job == "elsewhere":            # profile level 2, the culled engine, a gate: never a solo pass
        ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=2)
        out["profile2"] = one(ctx, big[:66000], tgt, 16)
        ctx.close()
        ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_PRUNED, profile=1)
        ctx.reset_profile()
        res, hist = ctx.align(big[:66000], tgt, capi.Context.make_config(max_iterations=16, tolerance=0.0, min_error=0.0))
        out["culled"] = {"T": hexes(res.transformation[:]), "hist": hexes(hist), "solo": int(ctx.get_profile()["nn_solo_passes"])}
        ctx.close()
        ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
        ctx.reset_profile()
        res, hist, kept = ctx.align_gated(big[:66000], tgt, capi.Context.make_config(max_iterations=16, tolerance=0.0, min_error=0.0), 0.5)
        out["gated"] = {"T": hexes(res.transformation[:]), "hist": hexes(hist), "kept": int(kept), "solo": int(ctx.get_profile()["nn_solo_passes"])}
        ctx.close()
print(json.dumps(out))
"""

_LEGS = {}
_KNOBS = ("ICPMI_NN_REUSE", "ICPMI_NN_MARGIN", "ICPMI_NN_LEAN", "ICPMI_NN_LEAN_FROM", "ICPMI_FUSE_FINISH", "ICPMI_NN_SOLO", "ICPMI_NN_SOLO_FROM",
          "ICPMI_NN_CULL_FULL", "ICPMI_NN_BOUNDED")


def _leg(jobs, tols=None, **env_extra):
    """One child process: the jobs under one setting of the knobs.  Run once and shared by the tests below."""
    key = (jobs, json.dumps(tols, sort_keys=True), tuple(sorted(env_extra.items())))
    if key not in _LEGS:
        env = dict(os.environ, ICPMI_SMALL="0", **env_extra)
        for k in _KNOBS:
            if k not in env_extra:
                env.pop(k, None)
        args = [sys.executable, "-c", _CHILD, ROOT, jobs] + ([json.dumps(tols)] if tols else [])
        r = subprocess.run(args, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        _LEGS[key] = json.loads(r.stdout.strip().splitlines()[-1])
    return _LEGS[key]


RESULT = ("T", "hist", "iters", "conv", "final", "nm", "idx", "cur")
STATS = ("rows", "blocks", "cert", "unmatched")
SIZES = (65472, 65473, 131072, 131073)
_MAIN = "per_pass16," + ",".join("size%d" % n for n in SIZES) + ",edge,elsewhere"


def _same(a, b, keys=RESULT):
    return [k for k in keys if a[k] != b[k]]


def _default():
    return _leg(_MAIN)


def _reference():
    return _leg(_MAIN + ",per_pass10", ICPMI_NN_SOLO="0")


def _forced():
    return _leg("per_pass10,edge", ICPMI_NN_SOLO_FROM="3")


def _rule(cert, n, passes):
    """The loop passes (from 1, of `passes` queued) whose tail the rule makes a solo kernel, from the rows certified per pass:
    solo_next (loop_plan.h) restated -- the counts of passes P - 3 and P - 2 are the latest the host has read."""
    uncert = [n - c for c in cert]
    return [P for P in range(6, passes + 1) if uncert[P - 4] == 0 and uncert[P - 3] == 0]


def test_solo_passes_change_no_bit_at_66000_rows():
    """The default against ICPMI_NN_SOLO=0 after calls of 1 .. 16 iterations (rings' edges: 1, 2, 3, 9): results, the normal
    matrix, the matches and moved rows of every pass, the rows listed and certified per pass, the lean passes; solo passes
    did run, and they are the passes the rule gives for the counts the call reports."""
    new, ref = _default()["per_pass16"], _reference()["per_pass16"]
    for k in range(1, 17):
        bad = _same(new[str(k)], ref[str(k)], RESULT + STATS)
        assert not bad, (k, bad)
        assert ref[str(k)]["prof"]["nn_solo_passes"] == 0 and ref[str(k)]["prof"]["nn_solo_fallback_rows"] == 0
        for c in ("nn_lean_passes", "bounded_launches", "nn_coarse_blocks", "nn_coarse_skipped", "nn_rows_listed", "nn_rows_certified"):
            assert new[str(k)]["prof"][c] == ref[str(k)]["prof"][c], (k, c)
        assert new[str(k)]["iters"] == k
        assert new[str(k)]["prof"]["nn_solo_passes"] == len(_rule(new[str(k)]["cert"], 66000, k)), k
    last = new["16"]
    print("certified per pass", last["cert"], "solo passes", last["prof"]["nn_solo_passes"], "searched by them", last["prof"]["nn_solo_fallback_rows"])
    assert last["cert"][7:] == [66000] * 10 and last["cert"][6] < 66000   # every row certified from pass 8 on ...
    assert _rule(last["cert"], 66000, 16) == list(range(11, 17))          # ... so the tail of pass 11 is the first solo kernel
    assert last["prof"]["nn_solo_passes"] == 6 and last["prof"]["nn_solo_fallback_rows"] == 0


@pytest.mark.parametrize("n", SIZES)
def test_edges_of_the_window(n):
    """65,472 and 131,073 rows: the plan is off and the counters are the reference's.  65,473 (1,024 partial rows, the last
    holding one valid row, 64 group rows) and 131,072 (128 workgroups): solo passes run.  Calls of 1, 2, 3, 9 and 16
    iterations and the last one twice, against ICPMI_NN_SOLO=0."""
    new, ref = _default()["size%d" % n], _reference()["size%d" % n]
    for k in ("1", "2", "3", "9", "16", "again"):
        assert new[k]["n"] == n
        bad = _same(new[k], ref[k], RESULT + STATS)
        assert not bad, (n, k, bad)
        assert new[k]["prof"]["nn_lean_passes"] == ref[k]["prof"]["nn_lean_passes"] and ref[k]["prof"]["nn_solo_passes"] == 0
        assert new[k]["prof"]["bounded_launches"] == ref[k]["prof"]["bounded_launches"]
    inside = 65473 <= n <= 131072
    passes = 16
    print(n, "certified per pass", new["16"]["cert"], "solo passes", new["16"]["prof"]["nn_solo_passes"])
    if inside:
        assert new["16"]["prof"]["nn_solo_passes"] == len(_rule(new["16"]["cert"], n, passes)) > 0
        assert new["again"]["prof"]["nn_solo_passes"] == new["16"]["prof"]["nn_solo_passes"]
        assert new["9"]["prof"]["nn_solo_passes"] == len(_rule(new["9"]["cert"], n, 9))
    else:
        for k in ("1", "2", "3", "9", "16", "again"):
            assert new[k]["prof"] == ref[k]["prof"], (n, k)


def test_forced_solo_passes_answer_by_their_own_search():
    """ICPMI_NN_SOLO_FROM=3 against ICPMI_NN_SOLO=0 over 1 .. 10 iterations: the tail of every pass from the third on is the
    solo kernel, tens of thousands of rows that are not certified take its exhaustive search, and results and the matches
    of every pass are the reference's.  (Per-pass statistics are not compared: see the module's docstring.)"""
    new, ref = _forced()["per_pass10"], _reference()["per_pass10"]
    for k in range(1, 11):
        bad = _same(new[str(k)], ref[str(k)], RESULT + ("unmatched",))
        assert not bad, (k, bad)
        assert new[str(k)]["prof"]["nn_solo_passes"] == max(0, k - 2), k
        assert new[str(k)]["prof"]["nn_lean_passes"] == max(0, k + 1 - 3), k   # the passes behind solo kernels are lean
    print("rows searched by solo kernels", new["10"]["prof"]["nn_solo_fallback_rows"], "certified per pass", new["10"]["cert"])
    assert new["10"]["prof"]["nn_solo_fallback_rows"] > 10000
    assert not _same(new["10"], new["again"]) and new["again"]["prof"]["nn_solo_passes"] == 8


def _tolerances():
    """From the reference history (the lean tests' construction): step[k] = |hist[k] - hist[k + 1]| is what iteration k + 2
    tests.  A tolerance between a record-low step and the smallest step before it ends the loop in that step's iteration."""
    hist = [float.fromhex(h) for h in _reference()["per_pass16"]["16"]["hist"]]
    step = [abs(hist[k] - hist[k + 1]) for k in range(16)]
    record = [k for k in range(16) if k == 0 or step[k] < min(step[:k])]
    late = [k for k in record if k + 2 >= 6]
    assert late, (record, step)
    k = late[0]
    return k + 2, (min(step[:k]) if step[k] == 0.0 else (step[k] * min(step[:k])) ** 0.5)


def test_stopping_test_inside_solo_mode():
    """A tolerance that ends the loop in iteration 6 or later with solo kernels from the fourth pass on (ICPMI_NN_SOLO_FROM=4:
    kernels queued behind the end find the loop done), and the smallest positive tolerance under the rule, wherever that
    ends; against ICPMI_NN_SOLO=0."""
    it, tol = _tolerances()
    tols = {"late": float.hex(tol), "tiny": float.hex(5e-324)}
    ref = _leg("tol", tols, ICPMI_NN_SOLO="0")["tol"]
    new = _leg("tol", tols)["tol"]
    forced = _leg("tol", tols, ICPMI_NN_SOLO_FROM="4")["tol"]
    assert ref["late"]["conv"] == 1 and ref["late"]["iters"] == it, (it, ref["late"]["iters"])
    print("ends in iterations", {k: v["iters"] for k, v in ref.items()}, "solo passes, rule", {k: v["prof"]["nn_solo_passes"] for k, v in new.items()},
          "forced", {k: v["prof"]["nn_solo_passes"] for k, v in forced.items()})
    for name in tols:
        assert not _same(new[name], ref[name]), name
        assert not _same(forced[name], ref[name]), name
    assert forced["late"]["prof"]["nn_solo_passes"] > 0   # the loop ended inside solo mode


def test_two_calls_on_one_context():
    """The same call twice on one context: the same bits and the same solo passes, in every leg."""
    for leg, job, k in ((_default(), "per_pass16", "16"), (_reference(), "per_pass16", "16"), (_forced(), "per_pass10", "10")):
        a, b = leg[job][k], leg[job]["again"]
        assert not _same(a, b, RESULT + STATS), job
        assert a["prof"] == b["prof"], job
    assert not _same(_default()["per_pass16"]["again"], _reference()["per_pass16"]["again"], RESULT + STATS)


def test_ties_and_nonfinite_rows():
    """Exact four-way ties (a tie never certifies: the hook's kernels search those rows and must break the ties as the listed
    path does; under the rule the solo passes are the ones the counts give) and a source with a NaN and an Inf row (a NaN pose from the first step on: idx = -1,
    terms from target 0), under the rule and forced from the third pass on."""
    ref = _reference()
    for leg in (_default(), _forced()):
        for name in ("ties", "nonfinite"):
            for k in ref[name]:
                assert not _same(leg[name][k], ref[name][k], RESULT + ("unmatched",)), (name, k)
    ties = _default()["ties"]["12"]
    print("ties: certified per pass", ties["cert"], "solo passes", ties["prof"]["nn_solo_passes"])
    assert ties["prof"]["nn_solo_passes"] == len(_rule(ties["cert"], ties["n"], 12))
    assert _default()["nonfinite"]["10"]["prof"]["nn_solo_passes"] == 0   # (rows under a NaN pose are never certified)
    assert _forced()["ties"]["12"]["prof"]["nn_solo_passes"] == 10 and _forced()["ties"]["12"]["prof"]["nn_solo_fallback_rows"] > 0
    assert ref["ties"]["12"]["unmatched"] == 0 and ref["nonfinite"]["1"]["unmatched"] == 66000
    assert _forced()["nonfinite"]["10"]["prof"]["nn_solo_passes"] == 8


@pytest.mark.parametrize("knob", ["ICPMI_NN_MARGIN", "ICPMI_NN_LEAN", "ICPMI_FUSE_FINISH"])
def test_solo_passes_stay_off_without_what_they_build_on(knob):
    """Without the match margin, lean passes or the fused tail: no solo pass, and the bits of ICPMI_NN_SOLO=0."""
    off = _leg("once16", **{knob: "0"})["once16"]
    assert off["prof"]["nn_solo_passes"] == 0 and off["prof"]["nn_solo_fallback_rows"] == 0
    assert not _same(off, _reference()["per_pass16"]["16"])
    assert not _same(off, _leg("once16", **{knob: "0", "ICPMI_NN_SOLO": "0"})["once16"], RESULT + STATS + ("prof",))


def test_solo_passes_stay_off_elsewhere():
    """Profile level 2 (the stage brackets want the three launches), the culled engine and a gated loop: no solo pass, and the
    bits of ICPMI_NN_SOLO=0."""
    new, ref = _default(), _reference()
    assert new["profile2"]["prof"]["nn_solo_passes"] == 0
    assert not _same(new["profile2"], ref["profile2"], RESULT + STATS + ("prof",))
    assert not _same(new["profile2"], ref["per_pass16"]["16"])
    for name in ("culled", "gated"):
        assert new[name]["solo"] == 0 and new[name] == ref[name], name
