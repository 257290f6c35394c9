"""The match margin of the bounded ICP passes (list_reuse.h "the match margin", RowBounds in kernels.h,
k_nn_resolve_bounded<true> in nn_bounded.h): a row whose kept match is certified as the unique nearest target is neither
listed nor scanned.  The registration must not change in any bit: every case runs in two child processes, one with the
margin (the default) and one with ICPMI_NN_MARGIN=0, on the all-pairs engine with ICPMI_SMALL=0, and pose, error
history, iteration count, flag, final error and the matches of every pass are compared byte for byte.
Marked gpu: runs on the MI355X box only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The child: every case as a set of registrations on ONE context (so each call also meets what the call before left in the
# per-row buffers).  `per_pass` cases run with max_iterations = 1 .. K and no stopping test: the matches the loop leaves
# after each call are those of pass k (the post-loop pass).
_CHILD = r"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch  # noqa: F401
from lidar_slam_from_scratch_amd import capi, synth

def lattice(shape, step, seed):
    g = np.stack(np.meshgrid(*[np.arange(k, dtype=np.float64) * step for k in shape], indexing="ij"), -1).reshape(-1, 3)
    return g[np.random.default_rng(seed).permutation(g.shape[0])]

def cases():
    s, t, _ = synth.c3_uniform(40000, seed=21, perm_seed=22)
    yield "c3_40k", s, t, None, 14, 0.0, 0.0, True
    # just above the 32,768-row switch between the resolve kernels, ragged last wave (33003 = 16 * 2062 + 11) and workgroup
    s, t, _ = synth.c3_uniform(33003, seed=31, perm_seed=32)
    yield "c3_33003", s, t, None, 10, 0.0, 0.0, True
    s, t, _ = synth.c3_uniform(40000, seed=23, perm_seed=24)
    yield "jump", s, t, synth.make_transform([0.0, 0.0, 0.25], [2.5, -1.5, 0.3]), 16, 0.0, 0.0, True
    s, t, _ = synth.c3_uniform(36000, seed=25, perm_seed=26)
    yield "overflow", s, t, synth.make_transform([0.1, -0.05, 0.6], [30.0, -20.0, 4.0]), 8, 0.0, 0.0, True
    # exact ties: a lattice target and a shifted sub-lattice source (every row is equidistant from four targets)
    t = lattice((40, 40, 24), 1.0, 27)
    s = t[::2] + np.array([0.5, 0.5, 0.0])
    yield "ties", s, t, synth.make_transform([0.0, 0.0, 0.002], [0.01, 0.0, 0.0]), 6, 0.0, 0.0, True
    # ... and with more than 32,768 rows, so that the ties meet the margin's kernels
    t = lattice((48, 48, 32), 1.0, 27)
    s = t[::2] + np.array([0.5, 0.5, 0.0])
    yield "ties_big", s, t, synth.make_transform([0.0, 0.0, 0.002], [0.01, 0.0, 0.0]), 6, 0.0, 0.0, True
    # a target with duplicated points: a third of its points twice, far apart in index
    s, t, _ = synth.c3_uniform(36000, seed=33, perm_seed=34)
    t = np.concatenate([t, t[::3]])
    yield "dup", s, t, None, 8, 0.0, 0.0, True
    # a source with one NaN and one Inf row
    s, t, _ = synth.c3_uniform(36000, seed=35, perm_seed=36)
    s = s.copy(); s[1234, 1] = np.nan; s[30001, 2] = np.inf
    yield "nonfinite", s, t, None, 8, 0.0, 0.0, True
    # the quarter-wave resolve's sizes: nothing is certified there and nothing may differ
    s, t, _ = synth.c1_room_corner()
    yield "c1", s, t, None, 50, 1e-6, 1e-9, False
    s, t, _ = synth.c2_lidar_pair()
    yield "c2", s, t, None, 50, 1e-6, 1e-9, False
    # two different registrations one after the other (the 40k case again behind c2): state left over by the call before
    s, t, _ = synth.c3_uniform(40000, seed=21, perm_seed=22)
    yield "again", s, t, synth.make_transform([0.0, 0.0, 0.01], [0.05, 0.0, 0.0]), 12, 0.0, 0.0, False
    s, t, _ = synth.c3_uniform(40000, seed=23, perm_seed=24)
    yield "again2", s, t, None, 12, 0.0, 0.0, False

ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
out = {}
for name, src, tgt, T0, iters, tol, mine, per_pass in cases():
    ks = list(range(1, iters + 1)) if per_pass else [iters]
    for k in ks:
        cfg = capi.Context.make_config(max_iterations=k, tolerance=tol, min_error=mine, initial_transform=T0)
        res, hist = ctx.align(src, tgt, cfg)
        idx, cur, perm, ok = ctx.debug_loop_rows(src.shape[0])
        assert ok
        key = "%s_%d" % (name, k)
        out[key + "_T"] = np.array(res.transformation[:])
        out[key + "_hist"] = np.asarray(hist, dtype=np.float64)
        out[key + "_flags"] = np.array([res.num_iterations, res.converged], dtype=np.int64)
        out[key + "_final"] = np.array([res.final_error])
        out[key + "_idx"] = idx  # (in the loop's internal order of rows, the same in both runs)
        if k == ks[-1]:
            out["cert_" + name] = np.array(ctx.nn_margin_passes(), dtype=np.int64)
ctx.close()
np.savez(sys.argv[2], **out)
print("ok", len(out))
"""

# The child of the counter test: the 40k registration, 30 passes with profiling on.
_CHILD_COUNTS = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import torch  # noqa: F401
from lidar_slam_from_scratch_amd import capi, synth
src, tgt, _ = synth.c3_uniform(40000, seed=21, perm_seed=22)
ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
res, hist = ctx.align(src, tgt, capi.Context.make_config(max_iterations=30, tolerance=0.0, min_error=0.0))
rows, blocks = ctx.nn_reuse_passes()
p = ctx.get_profile()
print(json.dumps({"rows": [int(r) for r in rows], "cert": [int(c) for c in ctx.nn_margin_passes()],
                  "hist": [float.hex(float(h)) for h in hist], "nn_rows_certified": int(p["nn_rows_certified"]),
                  "nn_rows_listed": int(p["nn_rows_listed"]), "nn_recheck_queries": int(p["nn_recheck_queries"])}))
ctx.close()
"""

# The child of the sharded test: 80,000 rows cut into two ranks' 40,000 (threads of this process, dist.LocalGroup) -- each
# rank's loop runs k_nn_resolve_bounded and k_step_transform -- 12 passes and the post-loop pass.
_CHILD_SHARDED = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import torch  # noqa: F401
from lidar_slam_from_scratch_amd import capi, dist as icpdist, synth
src, tgt, _ = synth.c3_uniform(80000, seed=21, perm_seed=22)
cfg = lambda: capi.Context.make_config(max_iterations=12, tolerance=0.0, min_error=0.0)
group = icpdist.LocalGroup(2)
def body(rank):
    lo, hi = icpdist.shard_bounds(src.shape[0], 2, rank)
    c = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
    group.attach(c, rank)
    res, hist = c.align(src[lo:hi], tgt, cfg())
    cert = c.nn_margin_passes()
    rows, _ = c.nn_reuse_passes()
    c.comm_finalize(); c.close()
    return {"n": hi - lo, "T": [float.hex(v) for v in res.transformation[:]], "hist": [float.hex(float(v)) for v in hist],
            "cert": [int(x) for x in cert], "rows": [int(x) for x in rows]}
print(json.dumps({"ranks": group.run(body)}))
"""


def _run(code, args, margin, timeout=900, **extra):
    env = dict(os.environ, ICPMI_NN_MARGIN=margin, ICPMI_SMALL="0", **extra)
    env.pop("ICPMI_NN_REUSE", None)
    r = subprocess.run([sys.executable, "-c", code, ROOT] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


_COUNTS = {}


def _counts(margin, **extra):
    """The counter child's result for one setting, run once and shared by the tests below."""
    key = (margin, tuple(sorted(extra.items())))
    if key not in _COUNTS:
        _COUNTS[key] = json.loads(_run(_CHILD_COUNTS, [], margin, **extra).strip().splitlines()[-1])
    return _COUNTS[key]


def test_match_margin_changes_no_bit(tmp_path):
    on, off = str(tmp_path / "on.npz"), str(tmp_path / "off.npz")
    _run(_CHILD, [on], "1")
    _run(_CHILD, [off], "0")
    a, b = np.load(on), np.load(off)
    assert sorted(a.files) == sorted(b.files) and len(a.files) > 0
    for k in sorted(a.files):
        if k.startswith("cert_"):
            print(k, "on", a[k].tolist(), "off", b[k].tolist())
    bad = [k for k in a.files if not k.startswith("cert_") and
           (a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes())]
    assert not bad, bad[:20]
    # the margin did run where it can, and nowhere else: the =0 leg certifies nothing, nor do the quarter-wave resolve's sizes
    assert all(b[k].size == 0 for k in b.files if k.startswith("cert_"))
    assert a["cert_c1"].sum() == 0 and a["cert_c2"].sum() == 0
    for name in ("c3_40k", "c3_33003", "jump", "again", "again2"):
        c = a["cert_" + name]
        assert c[0] == 0 and c[1] == 0 and c.sum() > 0, (name, c)
    # the finite cases did register: no row is left without a match
    for k in a.files:
        if k.endswith("_idx") and not k.startswith("nonfinite"):
            assert (a[k] >= 0).all(), k
    # the NaN and the Inf row have no match in the first pass and their terms are NaN, as the reference's are: the pose is
    # NaN from the first step on, and no later pass matches or certifies any row -- in both legs alike
    assert (a["nonfinite_1_idx"] < 0).all() and a["cert_nonfinite"].sum() == 0


def test_sharded_run_is_bit_equal():
    on = json.loads(_run(_CHILD_SHARDED, [], "1").strip().splitlines()[-1])
    off = json.loads(_run(_CHILD_SHARDED, [], "0").strip().splitlines()[-1])
    r0, r1 = on["ranks"]
    print("rank certified", r0["cert"], r1["cert"], "listed", r0["rows"], r1["rows"])
    assert r0["T"] == r1["T"] and r0["hist"] == r1["hist"]
    assert [x["T"] for x in off["ranks"]] == [r0["T"], r1["T"]] and [x["hist"] for x in off["ranks"]] == [r0["hist"], r1["hist"]]
    for r, o in zip(on["ranks"], off["ranks"]):
        assert len(r["cert"]) == 13 and r["cert"][0] == 0 and r["cert"][1] == 0 and sum(r["cert"]) > 0, r["cert"]
        assert o["cert"] == [] and sum(r["rows"]) <= sum(o["rows"])


def test_counters_of_a_settled_registration():
    """Passes 1 and 2 certify no row; every pass from two after the history settles certifies all n;
    nn_rows_certified is the per-pass sum; the rows listed are no more than without the margin, whose leg certifies none and
    has the same history."""
    r, r0 = _counts("1"), _counts("0")
    n, cert, rows = 40000, r["cert"], r["rows"]
    print("certified", cert, "listed", rows, "listed without", r0["rows"], "slots scanned", r["nn_recheck_queries"], r0["nn_recheck_queries"])
    assert len(cert) == 31 == len(rows)
    assert cert[0] == 0 and cert[1] == 0, cert[:3]
    hist = np.array([float.fromhex(h) for h in r["hist"]])
    settled = int(np.nonzero(np.abs(hist - hist[-1]) > 1e-9 * hist[-1])[0].max()) + 1
    assert settled <= 20, (settled, hist)
    assert all(cert[p] == n for p in range(settled + 2, len(cert))), (settled, cert)
    assert r["nn_rows_certified"] == sum(cert)
    assert sum(rows) <= sum(r0["rows"]), (rows, r0["rows"])
    assert r0["cert"] == [] and r0["nn_rows_certified"] == 0 and r0["hist"] == r["hist"]


def test_unfused_mover_is_bit_equal():
    """ICPMI_FUSE_FINISH=0: k_transform moves the rows through the same RowBatch::finish -- the same history in every bit
    as its own ICPMI_NN_MARGIN=0 leg and as the fused loop, and the same rows certified per pass as the fused loop."""
    fused, on, off = _counts("1"), _counts("1", ICPMI_FUSE_FINISH="0"), _counts("0", ICPMI_FUSE_FINISH="0")
    assert on["hist"] == off["hist"] == fused["hist"]
    assert off["cert"] == [] and on["cert"] == fused["cert"] and on["rows"] == fused["rows"]
