"""CPU model of list reuse and the match margin (csrc/list_reuse.h): per bounded pass of one
registration, the rows the coarse pass lists and the rows the exact resolve scans, with the margin on and off.

The poses are the oracle's after k = 0 .. K iterations; a row's nearest and second nearest target come from a cKDTree.
The arithmetic restates list_radius / list_certified / list_cover / match_margin / match_certified with f = 0.5 and
loose = 8, as RowBatch::finish applies them; a call's first pass leaves no margin (NaN cover).  min(d2 scanned, cover) is
min(second nearest distance, cover) whatever else the listed slots hold, since anything scanned beyond the cover is
farther than the cover.  Lists are taken never to overflow (true on the C3 clouds).  Every certified row's kept match is
checked against the tree's nearest neighbour.

Usage: python scripts/match_margin_sim.py [n] [passes] [seed perm_seed]      (default: C3, 100000 rows, 31 passes)"""
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lidar_slam_from_scratch_amd import synth  # noqa: E402
from oracle import oracle  # noqa: E402

UP, DOWN = 1.0 + 1e-12, 1.0 - 1e-12
F, LOOSE = 0.5, 8.0


def norm(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def list_radius(sq, disp):
    skin = np.minimum(np.maximum(F * sq, 2.0 * disp), sq)
    return (sq + 2.0 * skin) * UP


def simulate(src, tgt, poses, margin):
    """poses[p]: the 4x4 pose at which pass p + 1 searches.  Returns (rows listed, rows scanned) per pass."""
    n = src.shape[0]
    tree = cKDTree(tgt)
    listed, scanned = [], []
    match = np.zeros(n, np.int64)
    xs, g = np.zeros((n, 3)), np.full(n, np.nan)
    xb, rb = np.zeros((n, 3)), np.full(n, np.nan)
    prev = None
    for p, T in enumerate(poses):
        y = src @ T[:3, :3].T + T[:3, 3]
        dd, jj = tree.query(y, k=2)
        if p == 0:
            match, scan = jj[:, 0].copy(), np.ones(n, bool)
            cover = np.full(n, np.nan)
            listed.append(n)
        else:
            sq = norm(y - tgt[match])
            with np.errstate(invalid="ignore"):
                cert = ((sq + norm(y - xs)) * UP < g) if margin else np.zeros(n, bool)
                assert (match[cert] == jj[cert, 0]).all(), "a certified row's kept match is not the nearest neighbour"
                d = norm(y - xb)
                rn = list_radius(sq, norm(y - prev))
                keep = ((sq + d) * UP <= rb) & (rb <= LOOSE * rn)
            again = ~cert & ~keep
            xb[again], rb[again] = y[again], rn[again]
            cover = np.where(keep, rb * DOWN - d * UP, rn * DOWN)
            scan = ~cert
            match[scan] = jj[scan, 0]
            listed.append(int(again.sum()))
        gnew = np.where(cover < dd[:, 1] * DOWN, cover, dd[:, 1] * DOWN)
        gnew[np.isnan(cover)] = np.nan
        xs[scan], g[scan] = y[scan], gnew[scan]
        scanned.append(int(scan.sum()))
        prev = y
    return listed, scanned


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 31
    if len(sys.argv) > 4:
        src, tgt, _ = synth.c3_uniform(n, seed=int(sys.argv[3]), perm_seed=int(sys.argv[4]))
    else:
        src, tgt, _ = synth.c3_uniform(n)
    threads = min(16, os.cpu_count() or 1)
    poses = [np.eye(4)]
    for k in range(1, passes):
        poses.append(oracle.icp_point_to_plane(src, tgt, max_iterations=k, tolerance=0.0, min_error=0.0, nthreads=threads).transformation)
    for margin in (False, True):
        listed, scanned = simulate(src, tgt, poses, margin)
        print("margin", "on " if margin else "off", "rows listed ", listed, "total", sum(listed))
        print("margin", "on " if margin else "off", "rows scanned", scanned, "total", sum(scanned))


if __name__ == "__main__":
    main()
