"""List reuse of the bounded ICP passes (RowBounds in kernels.h, nn_bounded.h): a row keeps its list of slots from one
pass to the next while its bound and its drift from where the list was built certify that a new list could hold nothing
the kept one lacks.  The registration must not change in any bit: every case below runs in two child processes, one
with list reuse (the default) and one with ICPMI_NN_REUSE=0 (every row listed again in every pass), on the all-pairs
engine, and pose, error history, iteration count, flag and the matches of every pass are compared byte for byte.
Marked gpu: runs on the MI355X box only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The child: every case as a set of registrations on the all-pairs engine.  `per_pass` cases are run with max_iterations
# = 1 .. K and no stopping test, so that the matches the loop leaves after each call are those of pass k (the post-loop
# pass); the others once with their own configuration.  ICPMI_SMALL=0: C1 and C2 take the general kernels (the small-cloud
# kernel has no bounded passes).
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
    s, t, _ = synth.c1_room_corner()
    yield "c1", s, t, None, 50, 1e-6, 1e-9, True
    s, t, _ = synth.c2_lidar_pair()
    yield "c2", s, t, None, 50, 1e-6, 1e-9, False
    # a pose that jumps: far from the answer at first, so that the rows' drift varies across the cloud and some rows keep
    # their lists while others are listed again
    s, t, _ = synth.c3_uniform(40000, seed=23, perm_seed=24)
    yield "jump", s, t, synth.make_transform([0.0, 0.0, 0.25], [2.5, -1.5, 0.3]), 16, 0.0, 0.0, True
    # far outside the basin: every row's bound spans more slots than a list holds (the resolve's exhaustive path)
    s, t, _ = synth.c3_uniform(36000, seed=25, perm_seed=26)
    yield "overflow", s, t, synth.make_transform([0.1, -0.05, 0.6], [30.0, -20.0, 4.0]), 8, 0.0, 0.0, True
    # exact ties: a lattice target and a shifted sub-lattice source (every row is equidistant from four targets)
    t = lattice((40, 40, 24), 1.0, 27)
    s = t[::2] + np.array([0.5, 0.5, 0.0])
    yield "ties", s, t, synth.make_transform([0.0, 0.0, 0.002], [0.01, 0.0, 0.0]), 6, 0.0, 0.0, True

ctx = capi.Context(device=0, search=capi.SEARCH_MFMA_BF16, profile=0)
L = ctx._lib
L.icpmi_debug_loop_rows.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_int64]
out = {}
for name, src, tgt, T0, iters, tol, mine, per_pass in cases():
    ks = list(range(1, iters + 1)) if per_pass else [iters]
    for k in ks:
        cfg = capi.Context.make_config(max_iterations=k, tolerance=tol, min_error=mine, initial_transform=T0)
        res, hist = ctx.align(src, tgt, cfg)
        n = src.shape[0]
        idx, cur, perm = np.zeros(n, np.int32), np.zeros(3 * n), np.zeros(n, np.uint32)
        assert L.icpmi_debug_loop_rows(ctx._h, idx.ctypes.data_as(C.POINTER(C.c_int32)), cur.ctypes.data_as(C.POINTER(C.c_double)),
                                       perm.ctypes.data_as(C.POINTER(C.c_uint32)), n) == 0
        key = "%s_%d" % (name, k)
        out[key + "_T"] = np.array(res.transformation[:])
        out[key + "_hist"] = np.asarray(hist, dtype=np.float64)
        out[key + "_flags"] = np.array([res.num_iterations, res.converged], dtype=np.int64)
        out[key + "_final"] = np.array([res.final_error])
        out[key + "_idx"] = idx  # (in the loop's internal order of rows, the same in both runs)
ctx.close()
np.savez(sys.argv[2], **out)
print("ok", len(out))
"""

# The child of the counter test: one C3-like registration of 30 passes with profiling on.
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
print(json.dumps({"rows": rows, "blocks": blocks, "hist": [float(h) for h in hist], "bounded_launches": p["bounded_launches"],
                  "nn_rows_listed": p["nn_rows_listed"], "nn_coarse_skipped": p["nn_coarse_skipped"]}))
ctx.close()
"""


def _run(code, args, reuse, timeout=600):
    env = dict(os.environ, ICPMI_NN_REUSE=reuse, ICPMI_SMALL="0")
    r = subprocess.run([sys.executable, "-c", code, ROOT] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_list_reuse_changes_no_bit(tmp_path):
    on, off = str(tmp_path / "on.npz"), str(tmp_path / "off.npz")
    _run(_CHILD, [on], "1")
    _run(_CHILD, [off], "0")
    a, b = np.load(on), np.load(off)
    assert sorted(a.files) == sorted(b.files) and len(a.files) > 0
    bad = [k for k in a.files if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    assert not bad, bad[:20]
    # the cases did register: no row is left without a match in the cases with finite clouds
    for k in a.files:
        if k.endswith("_idx"):
            assert (a[k] >= 0).all(), k


def test_converged_passes_list_no_row():
    """On a converged C3-like registration the passes after convergence list no row again, and their coarse launches do
    no work; the first pass lists every row and the next one (whose bounds are the first pass's) too."""
    r = json.loads(_run(_CHILD_COUNTS, [], "1").strip().splitlines()[-1])
    rows, blocks = r["rows"], r["blocks"]
    n = 40000
    assert len(rows) == 31 == r["bounded_launches"], (len(rows), r["bounded_launches"])
    assert rows[0] == n and rows[1] == n, rows[:3]
    # converged: the error has settled to its last value well before the end of the loop
    hist = np.array(r["hist"])
    settled = int(np.nonzero(np.abs(hist - hist[-1]) > 1e-9 * hist[-1])[0].max()) + 1
    assert settled <= 20, (settled, hist)
    tail = range(settled + 2, len(rows))
    assert all(rows[p] == 0 for p in tail), (settled, rows)
    assert all(blocks[p] == 0 for p in tail), (settled, blocks)
    assert r["nn_coarse_skipped"] >= len(tail)
    assert r["nn_rows_listed"] == sum(rows)
    # and with ICPMI_NN_REUSE=0 nothing is counted (every pass lists every row, the form before list reuse)
    r0 = json.loads(_run(_CHILD_COUNTS, [], "0").strip().splitlines()[-1])
    assert r0["rows"] == [] and r0["nn_coarse_skipped"] == 0 and r0["hist"] == r["hist"]
