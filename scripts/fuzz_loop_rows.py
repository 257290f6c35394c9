#!/usr/bin/env python3
"""Every pass of the ICP loop against the exact fp64 nearest neighbour (run on the GPU box).

A registration is run once for each k = 1..K with no stopping test (tolerance = min_error = 0) and k - 1 iterations, so
that call k ends with pass k, the post-loop pass.  After each call the rows that pass matched are read back
(icpmi_debug_loop_rows: matches, moved rows, their order) and checked:

  (a) where the loop kept its matches: idx == exact_nn(target, cur) for every row with a finite cur, lowest index on ties;
  (b) on every path, the small-cloud kernel's included: the history's last entry equals sqrt(fsum(pd^2) / n) recomputed
      from the exact matches (pd = (dx*nx + dy*ny) + dz*nz, icp_oracle.c plane_rms), to (n + 64) * 2^-52 relative -- a
      bound on any order of summing n non-negative terms, while one wrong match moves it by about 1/n;
  (c) perm is a permutation of 0..n-1 and cur is the source in that order under the call's final pose.

The shapes come from the size thresholds that pick the loop's kernels (THRESHOLDS_N, THRESHOLDS_M), each plus
{-1, 0, +1, +31, +33}; a trial draws shape, geometry, engine and K at random.  Each failing row is printed with its true
match.
usage: python scripts/fuzz_loop_rows.py [trials] [first_seed]
       python scripts/fuzz_loop_rows.py case <n> <m> <geometry> <engine> <K> <seed> [no-error]   (one case; JSON last)"""
import json
import math
import os
import sys
import time

import numpy as np
import torch  # noqa: F401
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402

WORKERS = 16                      # CPU threads of the reference (never the machine's whole count)
GEOMETRIES = ("uniform", "lattice", "far", "clusters", "nonfinite")
ENGINES = {"auto": capi.SEARCH_AUTO, "mfma": capi.SEARCH_MFMA_BF16, "pruned": capi.SEARCH_MFMA_PRUNED,
           "exact": capi.SEARCH_EXACT_F64}
# capi.hip / nn_mfma.h / nn_culled.h / icp_small.h: kMfmaMinQueries, 4096 (sorted rows), kSmallMaxQueries, resolve layout,
# kBboxSingleMax; kMfmaMinTargets, 8 / 12 splits (small kernel, kAutoCulledFrom), kBboxSingleMax, kCullLdsBoxes splits
THRESHOLDS_N = (64, 4096, 32768, 65536)
THRESHOLDS_M = (256, 2048, 16384, 24576, 65536, 262144)


# ---- the reference ----------------------------------------------------------------------------------------------------

def sqdist(tgt, q):
    """The oracle's sqdist3 order, (dx*dx + dy*dy) + dz*dz, row by row."""
    d = tgt - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


class Reference:
    """Exact nearest neighbours in one target (a kd-tree over its finite rows, built once): nn(q) as exact_nn."""

    def __init__(self, tgt):
        from scipy.spatial import cKDTree
        self.tgt = np.ascontiguousarray(tgt, dtype=np.float64)
        self.fin = np.flatnonzero(np.isfinite(self.tgt).all(axis=1))
        self.tree = cKDTree(self.tgt[self.fin]) if self.fin.size else None

    def nn(self, q, k=16):
        tgt, fin, tree = self.tgt, self.fin, self.tree
        q = np.ascontiguousarray(q, dtype=np.float64)
        out = np.full(q.shape[0], -1, dtype=np.int64)
        rows = np.flatnonzero(np.isfinite(q).all(axis=1))
        if fin.size == 0 or rows.size == 0:
            return out
        k = min(k, fin.size)
        qr = q[rows]
        ds, js = tree.query(qr, k=np.arange(1, k + 1), workers=WORKERS)
        cand = fin[js]                                            # (rows, k) target indices, ascending kd-tree distance
        d2 = sqdist(tgt[cand], qr[:, None, :])
        best = d2.min(axis=1)
        big = np.iinfo(np.int64).max
        out[rows] = np.where(d2 == best[:, None], cand, big).min(axis=1)
        if k < fin.size:
            # the k-th candidate's distance is within the margin of the minimum: targets beyond it may tie, or be nearer
            wide = np.flatnonzero(ds[:, -1] * ds[:, -1] <= best * (1 + 1e-9))
            if wide.size:
                radius = np.sqrt(best[wide] * (1 + 1e-9)) * (1 + 1e-12) + 1e-300
                balls = tree.query_ball_point(qr[wide], radius, workers=WORKERS)
                for w, ball in zip(wide, balls):
                    c = fin[np.asarray(ball, dtype=np.int64)]
                    dd = sqdist(tgt[c], qr[w])
                    out[rows[w]] = c[dd == dd.min()].min()
        return out


def exact_nn(tgt, q):
    """For each row of q the lowest target index whose squared distance (sqdist3's order) is the minimum; targets with a
    non-finite coordinate are never matches, a row with one gets -1 (as does every row when no target is finite).
    Candidates come from a kd-tree over the finite targets; the minimum and its ties are decided on distances recomputed
    exactly, over the 16 nearest, or -- where the 16th is within 1e-9 of the minimum, so that more may tie or be nearer --
    over a ball slightly larger than that minimum."""
    return Reference(tgt).nn(q)


def plane_terms(cur, tgt, nrm, idx):
    """pd^2 per row, pd = (dx*nx + dy*ny) + dz*nz with d = target - row (icp_oracle.c plane_rms); the error of n rows is
    sqrt(fsum(pd^2) / n)."""
    d = tgt[idx] - cur
    nn = nrm[idx]
    pd = (d[:, 0] * nn[:, 0] + d[:, 1] * nn[:, 1]) + d[:, 2] * nn[:, 2]
    return pd * pd


def error_bound(n):
    """Relative distance between two sums of the same n non-negative terms in any two orders (plus the division and the
    square root): (n + 64) * 2^-52."""
    return (n + 64) * 2.0 ** -52


# ---- the cases --------------------------------------------------------------------------------------------------------

def _rot(rng, angle):
    axis = rng.normal(size=3)
    return axis / np.linalg.norm(axis) * angle


def geometry(kind, n, m, seed, offset=0.0):
    """(source, target, initial transform) of n -> m points.
      uniform    two independent samples of a 20 m box, a small motion: the loop converges and list reuse keeps lists
      lattice    integer lattice target with holes and duplicates, source on the shifted sub-lattice (i + 1/2, j + 1/2, k):
                 every row equidistant from four targets in the first pass
      far        uniform, started 30 m and 0.6 rad off: the rows' bounds span more slots than a list holds (exhaustive path)
      clusters   Gaussian clusters with far outliers (1e3 m) in both clouds
      nonfinite  uniform, with NaN and +-inf target rows"""
    rng = np.random.default_rng(seed)
    T0 = synth.make_transform(_rot(rng, 0.01), rng.normal(0, 0.05, 3))
    if kind in ("uniform", "far", "nonfinite"):
        tgt = rng.uniform(-10, 10, (m, 3))
        src = rng.uniform(-10, 10, (n, 3))
        if kind == "far":
            T0 = synth.make_transform(_rot(rng, 0.6), [30.0, -20.0, 4.0])
        if kind == "nonfinite":
            bad = rng.choice(m, max(3, m // 500), replace=False) if m >= 8 else np.arange(1)
            for j, b in enumerate(bad):
                tgt[b, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    elif kind == "lattice":
        side = max(2, int(math.ceil((1.25 * m) ** (1 / 3))))
        cells = np.stack(np.unravel_index(rng.choice(side ** 3, m, replace=m > side ** 3), (side,) * 3), -1).astype(np.float64)
        dup = rng.choice(m, m // 100, replace=False)
        cells[dup] = cells[rng.integers(0, m, dup.size)]      # exact duplicates
        tgt = cells
        sub = np.stack(np.unravel_index(rng.integers(0, (side - 1) ** 2 * side, n), (side - 1, side - 1, side)), -1)
        src = sub.astype(np.float64) + np.array([0.5, 0.5, 0.0])
        T0 = np.eye(4)
    elif kind == "clusters":
        centres = rng.uniform(-10, 10, (max(1, m // 400), 3))
        tgt = centres[rng.integers(0, centres.shape[0], m)] + rng.normal(0, 0.3, (m, 3))
        src = centres[rng.integers(0, centres.shape[0], n)] + rng.normal(0, 0.3, (n, 3))
        for c, cnt in ((tgt, m), (src, n)):
            far = rng.choice(cnt, max(1, cnt // 200), replace=False)
            c[far] = rng.uniform(-1, 1, (far.size, 3)) * 1e3
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(src + offset), np.ascontiguousarray(tgt + offset), T0


def reference_normals(tgt, kind, ctx=None):
    """The target normals for check (b): the oracle's, computed over the finite targets (the others are never anybody's
    neighbours).  On a lattice every row's 20th neighbour is tied, where the oracle's kd-tree and the library's lowest
    index rule legitimately pick different points (fuzz_engines.py): there the library's own estimate_normals (the
    kernels the loop runs, checked against the oracle elsewhere) is taken."""
    if kind == "lattice":
        return ctx.estimate_normals(tgt, 20)
    from oracle import oracle as orc
    fin = np.isfinite(tgt).all(axis=1)
    nrm = np.full(tgt.shape, np.nan)
    nrm[fin] = orc.estimate_normals(np.ascontiguousarray(tgt[fin]), None, 20, nthreads=WORKERS)
    return nrm


def check_pass(label, ref, nrm, T, hist, rows, n_total, want_err=True, log=print):
    """Checks (a)-(c) on one pass.  rows: list of (idx, cur, perm, idx_valid, source rows) per rank, n_total their rows
    together (the divisor of the error).  (b) is left out where a row is non-finite or no target is: there is no exact
    match to recompute the error from.  Returns (failures, whether idx was checked)."""
    bad = 0
    tgt = ref.tgt
    parts = []
    R, t = T[:3, :3], T[:3, 3]
    for r, (idx, cur, perm, valid, s) in enumerate(rows):
        n = s.shape[0]
        if not np.array_equal(np.sort(perm), np.arange(n, dtype=perm.dtype)):                         # (c)
            log("FAIL %s rank %d: perm is not a permutation of 0..%d" % (label, r, n - 1)); bad += 1
            continue
        moved = s[perm] @ R.T + t
        scale = 1.0 + np.abs(moved).max(initial=0.0)
        if n and not (np.abs(cur - moved).max() <= 1e-9 * scale):
            log("FAIL %s rank %d: cur is not the source in perm's order under the final pose (max diff %.3g)"
                % (label, r, np.abs(cur - moved).max())); bad += 1
            continue
        want = ref.nn(cur)
        fin = np.isfinite(cur).all(axis=1)
        if valid:                                                                                          # (a)
            diff = np.flatnonzero(fin & (idx != want))
            if diff.size:
                bad += 1
                log("FAIL %s rank %d: %d of %d rows matched a target other than the exact nearest"
                    % (label, r, diff.size, n))
                for row in diff[:8]:
                    p = cur[row]
                    dg = sqdist(tgt[idx[row]], p) if idx[row] >= 0 else float("nan")
                    log("   row %d (source row %d) p %s -> %d d2 %.17g   truth %d d2 %.17g"
                        % (row, perm[row], p.tolist(), idx[row], dg, want[row], sqdist(tgt[want[row]], p)))
        if not fin.all() or (want < 0).any():
            want_err = False
        else:
            parts.append((cur, want))
    if want_err and nrm is not None and len(parts) == len(rows):                                        # (b)
        e = math.sqrt(math.fsum(np.concatenate([plane_terms(cur, tgt, nrm, want) for cur, want in parts]).tolist())
                      / n_total)
        got = float(hist[-1])
        if not abs(got - e) <= error_bound(n_total) * max(abs(got), abs(e)):
            bad += 1
            log("FAIL %s: error %.17g against %.17g recomputed from the exact matches (relative %.3g, bound %.3g)"
                % (label, got, e, abs(got - e) / max(abs(e), 1e-300), error_bound(n_total)))
    return bad, all(row[3] for row in rows)


def run_case(ctx, src, tgt, T0, K, nrm, label, log=print):
    """Calls k = 1..K on `ctx` (k - 1 iterations, no stopping test), checks after each.  Returns a summary dict."""
    n = src.shape[0]
    out = {"label": label, "failures": 0, "idx_checked": 0, "error_only": 0, "sorted": False}
    ref = Reference(tgt)
    for k in range(1, K + 1):
        cfg = capi.Context.make_config(max_iterations=k - 1, tolerance=0.0, min_error=0.0, initial_transform=T0)
        res, hist = ctx.align(src, tgt, cfg)
        if hist.shape[0] != k:
            out["failures"] += 1
            log("FAIL %s pass %d: history of %d entries" % (label, k, hist.shape[0]))
            continue
        idx, cur, perm, valid = ctx.debug_loop_rows(n)
        out["sorted"] |= bool(n and (perm != np.arange(n)).any())
        T = np.array(res.transformation[:]).reshape(4, 4)
        bad, checked = check_pass("%s pass %d" % (label, k), ref, nrm, T, hist, [(idx, cur, perm, valid, src)], n,
                                  log=log)
        out["failures"] += bad
        out["idx_checked" if checked else "error_only"] += 1
    return out


def case(n, m, kind, engine, K, seed, offset=0.0, log=print, check_error=True):
    """One case on a fresh profiling context: the summary of run_case plus the profile counters of its calls.
    check_error=False leaves (b) out (no reference normals: targets of millions of points)."""
    src, tgt, T0 = geometry(kind, n, m, seed, offset)
    ctx = capi.Context(device=0, search=ENGINES[engine], profile=2)
    try:
        nrm = reference_normals(tgt, kind, ctx) if check_error else None
        ctx.reset_profile()
        out = run_case(ctx, src, tgt, T0, K, nrm, "%s %d->%d %s K=%d seed %d" % (engine, n, m, kind, K, seed), log=log)
        p = ctx.get_profile()
    finally:
        ctx.close()
    for f in ("small_launches", "bounded_launches", "coarse_launches", "nn_fallback_queries", "nn_group_pairs",
              "nn_group_pairs_run", "nn_rows_listed"):
        out[f] = int(p[f])
    return out


def main(argv=None):
    argv = list(sys.argv if argv is None else argv)
    if len(argv) > 1 and argv[1] == "case":
        n, m, kind, engine, K, seed = int(argv[2]), int(argv[3]), argv[4], argv[5], int(argv[6]), int(argv[7])
        out = case(n, m, kind, engine, K, seed, check_error="no-error" not in argv[8:])
        print(json.dumps(out))
        return 0 if out["failures"] == 0 else 1
    trials = int(argv[1]) if len(argv) > 1 else 40
    seed0 = int(argv[2]) if len(argv) > 2 else 1000
    deltas = (-1, 0, 1, 31, 33)
    bad = checked = err_only = 0
    t0 = time.time()
    for t in range(trials):
        seed = seed0 + t
        rng = np.random.default_rng(seed)
        n = max(1, int(rng.choice(THRESHOLDS_N)) + int(rng.choice(deltas)))
        m = max(1, int(rng.choice(THRESHOLDS_M)) + int(rng.choice(deltas)))
        kind = str(rng.choice(GEOMETRIES))
        engine = str(rng.choice(("auto", "mfma", "pruned")))
        K = int(rng.integers(1, 9))
        offset = float(rng.choice([0.0, 0.0, 0.0, 1e5]))
        out = case(n, m, kind, engine, K, seed, offset)
        bad += out["failures"] > 0
        checked += out["idx_checked"]
        err_only += out["error_only"]
        if out["failures"]:
            print("MISMATCH seed %d: %s" % (seed, json.dumps(out)))
    print("fuzz_loop_rows: %d trials, %d failing; passes with idx checked %d, error only %d; %.1f s"
          % (trials, bad, checked, err_only, time.time() - t0))
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
