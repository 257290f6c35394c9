"""Every pass of the ICP loop matches each row with its exact fp64 nearest target, lowest index on ties -- checked pass by
pass against scripts/fuzz_loop_rows.py's reference (a kd-tree's candidates decided on distances recomputed in the oracle's
order), not against another leg of the library.  Call k of a case runs k - 1 iterations with no stopping test, so that it
ends with pass k; after it the rows that pass matched are read back (icpmi_debug_loop_rows) and checked:
(a) the matches, where the loop keeps them; (b) the history's last entry against the error recomputed from the exact
matches, on every path; (c) the order of the rows (see fuzz_loop_rows.check_pass).

The shapes straddle the thresholds that pick the loop's kernels (capi.hip: kMfmaMinTargets / kMfmaMinQueries,
kSmallMaxQueries, 8 and 12 splits, resolve_waves, kSortRowsFromSplits, kCullMaxSplits; nn_mfma.h kBboxSingleMax;
nn_culled.h kCullLdsBoxes; icp_small.h kSmallQ / kSmallMaxSplits), one case at or under each limit and one past it, and
each runs a converging uniform pair and one hard geometry (lattice ties, a far start whose lists overflow to the
exhaustive path, clusters with far outliers, non-finite targets).  The profile counters show which path ran.
Marked gpu: runs on the MI355X box only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# (id, engine, n rows, m targets, hard geometry, the path the loop must take)
SHAPES = [
    ("exact_255", "auto", 5000, 255, "lattice", "exact"),              # kMfmaMinTargets
    ("mfma_256", "auto", 5000, 256, "nonfinite", "small"),
    ("exact_q63", "auto", 63, 20000, "clusters", "exact"),             # kMfmaMinQueries
    ("mfma_q64", "auto", 64, 20000, "far", "allpairs"),
    ("small_2049", "auto", 1000, 2049, "lattice", "small"),            # last split holds one target; kSmallQ tail
    ("small_4097", "auto", 4097, 16384, "nonfinite", "small"),         # 8 splits
    ("small_32768", "auto", 32768, 16384, "clusters", "small"),        # kSmallMaxQueries
    ("general_32769", "auto", 32769, 16384, "far", "allpairs"),
    ("allpairs_9_32768", "auto", 32768, 16385, "lattice", "allpairs"),  # 9 splits; resolve layout at 32,768 rows
    ("allpairs_9_32769", "auto", 32769, 16385, "far", "allpairs"),
    ("allpairs_12_half", "auto", 5000, 24576, "nonfinite", "allpairs"),  # 12 splits, half units
    ("culled_13", "auto", 5000, 24577, "far", "culled"),               # kAutoCulledFrom
    ("culled_13_40k", "auto", 40000, 24577, "lattice", "culled"),
    ("culled_bbox_65536", "auto", 20000, 65536, "clusters", "culled"),  # target kBboxSingleMax
    ("culled_bbox_65537", "auto", 20000, 65537, "nonfinite", "culled"),
    ("culled_rows_65536", "auto", 65536, 70000, "far", "culled"),      # row kBboxSingleMax
    ("culled_rows_65537", "auto", 65537, 70000, "lattice", "culled"),
    ("culled_lds_128", "auto", 20000, 262144, "clusters", "culled"),   # kCullLdsBoxes
    ("culled_lds_129", "auto", 20000, 262145, "far", "culled"),
    ("unsorted_4095", "mfma", 4095, 40000, "lattice", "allpairs"),     # kSortRowsFromSplits, n >= 4096
    ("sorted_4096", "mfma", 4096, 40000, "far", "sorted"),
    ("pruned_small_target", "pruned", 2000, 3000, "clusters", "culled"),
]
K = 6
SEED = 4100


def _check_path(out, path, kind):
    if path == "exact":
        assert out["small_launches"] == 0 and out["bounded_launches"] == 0 and out["nn_group_pairs"] == 0, out
    elif path == "small":
        assert out["small_launches"] > 0 and out["bounded_launches"] == 0, out
    else:
        assert out["small_launches"] == 0 and out["bounded_launches"] > 0, out
        assert (out["nn_group_pairs_run"] > 0) == (path == "culled"), out
        if kind == "far":   # the lists overflowed: rows went to the exhaustive path
            assert out["nn_fallback_queries"] > 0, out
    assert out["sorted"] == (path in ("culled", "sorted")), out
    # the small-cloud kernel keeps no matches: only (b) and (c) there
    assert (out["error_only"] == K) == (path == "small") and out["idx_checked"] + out["error_only"] == K, out


def _report(out):
    print("LOOP_MATCHES " + json.dumps(out))


@pytest.mark.parametrize("sid,engine,n,m,hard,path", SHAPES, ids=[s[0] for s in SHAPES])
def test_loop_matches_exact_nn(sid, engine, n, m, hard, path, oracle):
    import fuzz_loop_rows as F
    lines = []
    for i, kind in enumerate(("uniform", hard)):
        out = F.case(n, m, kind, engine, K, SEED + i, log=lines.append)
        _report(out)
        assert out["failures"] == 0, "\n".join(lines[:60])
        _check_path(out, path, kind)


def _child(args, env_extra, timeout):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_loop_rows.py"), "case"] + [str(a) for a in args],
                       env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    _report(out)
    return out


@pytest.mark.parametrize("m,hard,path", [(32768, "nonfinite", "small"), (32769, "far", "sorted")], ids=["16_splits", "17_splits"])
def test_loop_matches_small_kernel_lds_limit(m, hard, path, oracle):
    """ICPMI_SMALL_MAX_SPLITS=16 (read once per process: a child) puts the small-cloud kernel at kSmallMaxSplits, all its
    LDS records in use; one split more is the all-pairs engine's general kernels, rows sorted.  (The all-pairs engine
    named: AUTO would take the culled engine beyond 12 splits.)"""
    for i, kind in enumerate(("uniform", hard)):
        out = _child([20000, m, kind, "mfma", K, SEED + 10 + i], {"ICPMI_SMALL_MAX_SPLITS": "16"}, 900)
        _check_path(out, path, kind)


@pytest.mark.parametrize("m,kind,path", [(3072 * 2048, "uniform", "culled"), (3072 * 2048 + 1, "clusters", "sorted")],
                         ids=["3072_splits", "3073_splits"])
def test_loop_matches_past_the_cull_limit(m, kind, path, oracle):
    """kCullMaxSplits: a target of 3,072 splits is the culled engine's, one more target point all pairs (sorted rows).
    K = 2, the matches only (no oracle normals of 6.3M points), and one geometry per side: every call estimates the
    normals of the 6.3M-point target again, about 80 s a call."""
    out = _child([4096, m, kind, "auto", 2, SEED + 20 + (kind == "clusters"), "no-error"], {}, 900)
    assert out["failures"] == 0 and out["idx_checked"] == 2, out
    assert out["small_launches"] == 0 and out["bounded_launches"] > 0 and out["sorted"], out
    assert (out["nn_group_pairs_run"] > 0) == (path == "culled"), out


def test_loop_matches_two_ranks(oracle):
    """The sharded loop (two ranks as threads of this process, icpdist.LocalGroup; culled: 30 splits): each rank's rows
    against the exact matches, the shared history against the error of both ranks' rows together."""
    import fuzz_loop_rows as F
    from lidar_slam_from_scratch_amd import capi, dist as icpdist
    n, m = 60000, 60000
    for i, kind in enumerate(("uniform", "lattice")):
        src, tgt, T0 = F.geometry(kind, n, m, SEED + 30 + i)
        ref = F.Reference(tgt)
        one = capi.Context(device=0)
        nrm = F.reference_normals(tgt, kind, one)
        one.close()
        group = icpdist.LocalGroup(2)

        def body(rank):
            lo, hi = icpdist.shard_bounds(n, 2, rank)
            ctx = capi.Context(device=0, profile=2)
            group.attach(ctx, rank)
            got = []
            for k in range(1, K + 1):
                cfg = capi.Context.make_config(max_iterations=k - 1, tolerance=0.0, min_error=0.0, initial_transform=T0)
                res, hist = ctx.align(src[lo:hi], tgt, cfg)
                got.append((np.array(res.transformation[:]).reshape(4, 4), hist) + ctx.debug_loop_rows(hi - lo))
            p = ctx.get_profile()
            ctx.comm_finalize()
            ctx.close()
            return got, p
        r = group.run(body)
        lines = []
        for k in range(K):
            T, hist = r[0][0][k][:2]
            assert (r[1][0][k][0] == T).all() and (r[1][0][k][1] == hist).all() and hist.shape[0] == k + 1
            rows = []
            for rank in range(2):
                lo, hi = icpdist.shard_bounds(n, 2, rank)
                idx, cur, perm, valid = r[rank][0][k][2:]
                rows.append((idx, cur, perm, valid, src[lo:hi]))
            bad, checked = F.check_pass("two ranks %s pass %d" % (kind, k + 1), ref, nrm, T, hist, rows, n, log=lines.append)
            assert bad == 0 and checked, "\n".join(lines[:60])
        for rank in range(2):
            assert r[rank][1]["nn_group_pairs_run"] > 0, r[rank][1]   # the culled engine ran on both ranks
        _report({"label": "two ranks %s" % kind, "idx_checked": K, "error_only": 0})


def test_debug_loop_rows_status_and_order(oracle):
    """icpmi_debug_loop_rows tells what it has: after a small-cloud kernel call no matches (DEBUG_NO_IDX, idx all -1);
    after an unsorted call that follows a sorted one on the same AUTO context the identity order, not the earlier call's
    Morton order; after a nearest_batch call (which reuses the buffer) no matches; a row count other than the last
    registration's is an error."""
    import fuzz_loop_rows as F
    from lidar_slam_from_scratch_amd import capi
    ctx = capi.Context(device=0)
    cfg = capi.Context.make_config(max_iterations=2, tolerance=0.0, min_error=0.0)
    big_src, big_tgt, _ = F.geometry("uniform", 5000, 30000, 1)          # 15 splits: culled, rows sorted
    ctx.align(big_src, big_tgt, cfg)
    idx, cur, perm, valid = ctx.debug_loop_rows(5000)
    assert valid and (perm != np.arange(5000)).any() and (idx >= 0).all()
    src, tgt, _ = F.geometry("uniform", 3000, 10000, 2)                  # 5 splits: the small-cloud kernel
    ctx.align(src, tgt, cfg)
    idx, cur, perm, valid = ctx.debug_loop_rows(3000)
    assert not valid and (idx == -1).all() and (perm == np.arange(3000)).all()
    src, tgt, _ = F.geometry("uniform", 3000, 20000, 3)                  # 10 splits: all pairs, rows in the caller's order
    res, _ = ctx.align(src, tgt, cfg)
    idx, cur, perm, valid = ctx.debug_loop_rows(3000)
    assert valid and (perm == np.arange(3000)).all()
    T = np.array(res.transformation[:]).reshape(4, 4)
    assert np.abs(cur - (src @ T[:3, :3].T + T[:3, 3])).max() < 1e-9
    with pytest.raises(capi.IcpError):
        ctx.debug_loop_rows(2999)
    ctx.nearest_batch(tgt, src[:100])
    idx, cur, perm, valid = ctx.debug_loop_rows(3000)
    assert not valid and (idx == -1).all()
    ctx.close()
