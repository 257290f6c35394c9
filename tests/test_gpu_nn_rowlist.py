"""The packed list of the rows listed again (RowBounds::mask and k_row_list in kernels.h, RowsListed in nn_mfma.h): with
list reuse the coarse pass of the all-pairs engine runs over the rows that were listed again and over no others, so the
workgroup columns a pass runs are ceil(rows listed / 512) -- not every 512-row block that holds one such row.  The work
runs in child processes (reuse on, and ICPMI_NN_REUSE=0 as the reference leg).  Marked gpu: runs on the MI355X box only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The child of the counter test: 30 passes with profiling on, on the C3-like 40k case and on the 100k C3 pair.
_CHILD_COUNTS = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import torch  # noqa: F401
from lidar_slam_from_scratch_amd import capi, synth
out = {}
for name, (src, tgt, _) in (("c3_40k", synth.c3_uniform(40000, seed=21, perm_seed=22)), ("c3_100k", synth.c3_uniform())):
    ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
    res, hist = ctx.align(src, tgt, capi.Context.make_config(max_iterations=30, tolerance=0.0, min_error=0.0))
    rows, blocks = ctx.nn_reuse_passes()
    p = ctx.get_profile()
    out[name] = {"n": int(src.shape[0]), "rows": [int(r) for r in rows], "blocks": [int(b) for b in blocks],
                 "hist": [float.hex(float(h)) for h in hist], "nn_rows_listed": int(p["nn_rows_listed"]),
                 "nn_coarse_skipped": int(p["nn_coarse_skipped"]), "bounded_launches": int(p["bounded_launches"])}
    ctx.close()
print(json.dumps(out))
"""

# The child of the sharded test: the 40k case on one context, then cut into two ranks' rows (threads of this process,
# dist.LocalGroup), 12 passes and the post-loop pass each.
_CHILD_SHARDED = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import torch  # noqa: F401
from lidar_slam_from_scratch_amd import capi, dist as icpdist, synth
src, tgt, _ = synth.c3_uniform(40000, seed=21, perm_seed=22)
cfg = lambda: capi.Context.make_config(max_iterations=12, tolerance=0.0, min_error=0.0)
one = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16)
res1, hist1 = one.align(src, tgt, cfg())
one.close()
group = icpdist.LocalGroup(2)
def body(rank):
    lo, hi = icpdist.shard_bounds(src.shape[0], 2, rank)
    c = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=1)
    group.attach(c, rank)
    res, hist = c.align(src[lo:hi], tgt, cfg())
    rows, blocks = c.nn_reuse_passes()
    c.comm_finalize(); c.close()
    return {"n": hi - lo, "T": [float.hex(v) for v in res.transformation[:]], "hist": [float.hex(float(v)) for v in hist],
            "rows": [int(r) for r in rows], "blocks": [int(b) for b in blocks]}
r = group.run(body)
print(json.dumps({"one": {"T": [float.hex(v) for v in res1.transformation[:]], "hist": [float.hex(float(v)) for v in hist1]},
                  "ranks": r}))
"""


def _run(code, reuse, timeout=900):
    env = dict(os.environ, ICPMI_NN_REUSE=reuse, ICPMI_SMALL="0")
    r = subprocess.run([sys.executable, "-c", code, ROOT], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_a_pass_runs_the_columns_of_its_listed_rows_only():
    """blocks[p] == ceil(rows[p] / 512) in every pass p >= 1 (512: the rows of a workgroup at these sizes), on both cases;
    the history is that of ICPMI_NN_REUSE=0 in every bit."""
    on, off = _run(_CHILD_COUNTS, "1"), _run(_CHILD_COUNTS, "0")
    for name in ("c3_40k", "c3_100k"):
        r, n = on[name], on[name]["n"]
        rows, blocks = r["rows"], r["blocks"]
        print(name, "rows", rows, "blocks", blocks)
        assert len(rows) == len(blocks) == 31 == r["bounded_launches"]
        assert rows[0] == n and rows[1] == n and blocks[0] == -(-n // 512)
        bad = [(p, rows[p], blocks[p]) for p in range(1, len(rows)) if blocks[p] != -(-rows[p] // 512)]
        assert not bad, bad
        # the packed form did run: some pass listed a part of the rows, and some none
        assert any(0 < x < n for x in rows[2:]) and any(x == 0 for x in rows[2:]), rows
        assert r["nn_rows_listed"] == sum(rows)
        assert r["nn_coarse_skipped"] == sum(1 for p in range(1, len(rows)) if blocks[p] == 0)
        assert off[name]["rows"] == [] and off[name]["hist"] == r["hist"], name


def test_sharded_run_gives_the_unsharded_history():
    """Two ranks (k_step_transform leaves the words of each rank's rows): both ranks return the same bits, which are those
    of the same sharded run with ICPMI_NN_REUSE=0, and the unsharded run's history and pose up to the order of the fp64
    sums -- a rank's partial sums are added in another grouping, which moves a sum of n terms by at most n 2^-53 of its
    size per pass: passes x n x 2^-53, relative, is the bound (the loop contracts, so a pass does not amplify the one
    before).  Each rank's passes run ceil(rows / 512) workgroup columns."""
    on, off = _run(_CHILD_SHARDED, "1"), _run(_CHILD_SHARDED, "0")
    r0, r1 = on["ranks"]
    assert r0["T"] == r1["T"] and r0["hist"] == r1["hist"]
    assert [x["T"] for x in off["ranks"]] == [r0["T"], r1["T"]] and [x["hist"] for x in off["ranks"]] == [r0["hist"], r1["hist"]]
    assert on["one"] == off["one"]
    for r in (r0, r1):
        rows, blocks, n = r["rows"], r["blocks"], r["n"]
        print("rank rows", rows, "blocks", blocks)
        assert len(rows) == 13 and rows[0] == n and rows[1] == n
        assert all(blocks[p] == -(-rows[p] // 512) for p in range(1, len(rows))), (rows, blocks)
        assert any(0 < x < n for x in rows[2:]), rows
    h = np.array([float.fromhex(v) for v in r0["hist"]])
    h1 = np.array([float.fromhex(v) for v in on["one"]["hist"]])
    bound = 13 * 40000 * 2.0 ** -53
    print("sharded against unsharded, largest relative difference", np.abs(h / h1 - 1.0).max(), "bound", bound)
    assert h.shape == h1.shape == (13,)
    np.testing.assert_allclose(h, h1, rtol=bound, atol=0)
    T = np.array([float.fromhex(v) for v in r0["T"]])
    T1 = np.array([float.fromhex(v) for v in on["one"]["T"]])
    np.testing.assert_allclose(T, T1, rtol=0, atol=bound * max(1.0, np.abs(T1).max()))
