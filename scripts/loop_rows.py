"""Diagnostic: the per-row matches the ICP loop's last pass left behind, bounded form (nn_bounded.h) against unbounded
form, for one seed of scripts/fuzz_bounded.py (icpmi_debug_loop_rows exports them).  Every row whose match differs is
printed with both distances and the brute-force truth.
    python scripts/loop_rows.py <seed> [iterations]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
import torch  # noqa: F401
from lidar_slam_from_scratch_amd import capi
from fuzz_bounded import make_case as make

seed = int(sys.argv[1])
src, tgt, iters, tol, info = make(seed)
if len(sys.argv) > 2:
    iters = int(sys.argv[2])
print(seed, info, "iterations", iters)
n = src.shape[0]
out = {}
for knob in ("1", "0"):
    os.environ["ICPMI_NN_BOUNDED"] = knob
    ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16)
    res, hist = ctx.align(src, tgt, capi.Context.make_config(iters, 0.0, 0.0))
    idx, cur, perm, idx_valid = ctx.debug_loop_rows(n)
    assert idx_valid, "the small-cloud kernel ran this registration: it keeps no matches (ICPMI_SMALL=0 for the general kernels)"
    out[knob] = (idx, cur, perm, hist)
    print("knob", knob, "history", [float("%.9g" % h) for h in hist])
    ctx.close()
(i1, c1, p1, _), (i0, c0, p0, _) = out["1"], out["0"]
print("rows moved identically:", bool(np.array_equal(c1, c0, equal_nan=True)), " same order:", bool((p1 == p0).all()))
diff = np.nonzero(i1 != i0)[0]
print(len(diff), "rows with different matches")
for r in diff[:12]:
    p = c1[r]
    d = ((tgt - p) ** 2).sum(1)
    best = d.min(); where = np.nonzero(d == best)[0]
    print(" row", r, "src row", p1[r], "p", p, "bounded ->", i1[r], d[i1[r]] if i1[r] >= 0 else None, " unbounded ->", i0[r],
          d[i0[r]] if i0[r] >= 0 else None, " truth: d", best, "lowest index", where[0], "(%d tied)" % len(where))
