"""scripts/local_map_ref.py -- the CPU restatement of the local map (csrc/local_map.h, icpmi_local_map) and
of the scan-to-local-map driver (odometry.run_odometry_local_map) that tests/test_local_map_reference.py and
tests/test_gpu_local_map.py hold the library to.  The table must come out byte for byte.

The table: sorted unique 63-bit voxel keys (uint64) and one fp64 point per key.  In unfused fp64 and in this order:

    world point  p_a = ((x R_a0 + y R_a1) + z R_a2) + t_a                    (Rigid34::apply)
    cell         f_a = floor(p_a / voxel_size), accepted iff -2^20 <= f_a < 2^20 on every axis (a NaN or an infinity
                 fails the comparison); c_a = (int64)f_a
    key          (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20)
    range        d = p - t; d2 = (dx*dx + dy*dy) + dz*dz; in range iff d2 <= max_range*max_range
    dropped      a row whose cells are not accepted or that is out of range

    add(scan, pose):
        evict    residents out of range of this pose leave
        insert   among the rows not dropped, the lowest scan row of each voxel, if its key is not a surviving resident's
                 (an evicted resident's voxel is taken again by this scan's row); the others are merged away
        merge    survivors and insertions, sorted by key
        count    inserted + dropped + merged == n; rows == rows before - evicted + inserted
        an add whose result would exceed `capacity` rows raises CapacityError and leaves the table as it was

    LocalMapRef(voxel_size, max_range, capacity)    .add(scan, pose) -> dict of counts, .points() -> (points, keys)
    run_local_map(frames, align, ...)               the driver, with a pluggable aligner -> OdometryTrack
    oracle_align(), robust_align(kind, scale)       the oracle, or robust_icp_ref.robust_icp, as that aligner
    python scripts/local_map_ref.py [--long]        the drift table of DESIGN 7.11 (--long adds the 40-frame DRIVE_200 row)"""
import os
import sys
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

CELL_LIMIT = 1 << 20


class CapacityError(RuntimeError):
    pass


def world_points(scan, pose):
    """Rigid34::apply, row by row"""
    s = np.ascontiguousarray(scan, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(pose, dtype=np.float64).reshape(4, 4)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((x * T[a, 0] + y * T[a, 1]) + z * T[a, 2]) + T[a, 3] for a in range(3)], axis=1)


def in_range(points, t, r2):
    with np.errstate(all="ignore"):
        d = points - t
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return d2 <= r2


def keys_of(points, voxel_size):
    """-> (accepted mask, uint64 keys; 0 where not accepted)"""
    with np.errstate(all="ignore"):
        f = np.floor(points / voxel_size)
        ok = np.all((f >= -float(CELL_LIMIT)) & (f < float(CELL_LIMIT)), axis=1)
    c = np.zeros(f.shape, dtype=np.int64)
    c[ok] = f[ok].astype(np.int64) + CELL_LIMIT
    u = c.astype(np.uint64)
    return ok, (u[:, 0] << np.uint64(42)) | (u[:, 1] << np.uint64(21)) | u[:, 2]


class LocalMapRef:
    def __init__(self, voxel_size=0.5, max_range=100.0, capacity=1 << 20):
        self.voxel_size, self.max_range, self.capacity = float(voxel_size), float(max_range), int(capacity)
        self.keys = np.zeros(0, dtype=np.uint64)
        self.pts = np.zeros((0, 3))

    def size(self):
        return int(self.keys.shape[0])

    def points(self):
        return self.pts.copy(), self.keys.copy()

    def clear(self):
        self.keys, self.pts = np.zeros(0, dtype=np.uint64), np.zeros((0, 3))

    def add(self, scan, pose):
        T = np.asarray(pose, dtype=np.float64).reshape(4, 4)
        t = T[:3, 3].copy()
        r2 = self.max_range * self.max_range
        w = world_points(scan, T)
        n = w.shape[0]
        ok, keys = keys_of(w, self.voxel_size)
        ok &= in_range(w, t, r2)
        survive = in_range(self.pts, t, r2)                              # evict
        res_keys, res_pts = self.keys[survive], self.pts[survive]
        rows = np.flatnonzero(ok)
        ukeys, first = np.unique(keys[rows], return_index=True)           # the lowest scan row of each voxel
        fresh = ~np.isin(ukeys, res_keys)                                 # ... whose key no surviving resident holds
        new_keys, new_pts = ukeys[fresh], w[rows[first[fresh]]]
        total = res_keys.shape[0] + new_keys.shape[0]
        if total > self.capacity:
            raise CapacityError("the add would leave %d rows; the local map holds %d" % (total, self.capacity))
        all_keys = np.concatenate([res_keys, new_keys])
        order = np.argsort(all_keys, kind="stable")                       # merge
        info = dict(rows=total, inserted=int(new_keys.shape[0]), evicted=int(self.keys.shape[0] - res_keys.shape[0]),
                    dropped=int(n - rows.shape[0]))
        info["merged"] = n - info["inserted"] - info["dropped"]
        self.keys, self.pts = all_keys[order], np.concatenate([res_pts, new_pts])[order]
        return info


def invert(T):
    """(R^T, -R^T t)"""
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def oracle_align(orc=None, nthreads=4):
    """the oracle as run_local_map's aligner: (source, target, max_iterations, tolerance, initial_transform) -> result"""
    if orc is None:
        from oracle import oracle as orc
    return lambda s, t, it, tol, guess: orc.icp_point_to_plane(s, t, max_iterations=it, tolerance=tol, initial_transform=guess,
                                                               nthreads=nthreads)


def robust_align(kind, scale, max_distance=0.0, orc=None):
    """robust_icp_ref.robust_icp as the aligner"""
    import robust_icp_ref as rr
    return lambda s, t, it, tol, guess: rr.robust_icp(s, t, kind, scale, max_distance, it, tol, initial_transform=guess, orc=orc)


def run_local_map(frames, align, voxel_size=0.5, max_range=100.0, capacity=1 << 20, max_iterations=50, tolerance=1e-6,
                  min_points=1000, motion_model=True, on_frame=None):
    """odometry.run_odometry_local_map on the CPU.  on_frame(k, table, guess, result): called after frame k's add
    (guess and result None for frame 0 and for a frame of too few points).  -> OdometryTrack with map_rows."""
    from lidar_slam_from_scratch_amd.odometry import OdometryTrack
    track = OdometryTrack()
    track.map_rows = []
    table = LocalMapRef(voxel_size, max_range, capacity)
    delta = np.eye(4)
    for k, curr in enumerate(frames):
        curr = np.ascontiguousarray(curr, dtype=np.float64)
        t0 = time.perf_counter()
        if k == 0:
            table.add(curr, np.eye(4))
            track.map_rows.append(table.size())
            if on_frame:
                on_frame(k, table, None, None)
            continue
        prev = track.poses[-1]
        if curr.shape[0] < min_points:
            delta = np.eye(4)
            track.poses.append(prev.copy())
            track.deltas.append(delta)
            track.final_errors.append(float("nan"))
            track.iterations.append(0)
            track.converged.append(False)
            track.gated.append(True)
            track.map_rows.append(table.size())
            track.frame_ms.append(1e3 * (time.perf_counter() - t0))
            if on_frame:
                on_frame(k, table, None, None)
            continue
        guess = prev @ delta if motion_model else prev.copy()
        r = align(curr, table.pts, max_iterations, tolerance, guess)
        bad = (not r.converged) or r.final_error > 1.0
        pose = guess if bad else np.asarray(r.transformation, dtype=np.float64).reshape(4, 4)
        delta = invert(prev) @ pose
        table.add(curr, pose)                                             # always: a map that skips a frame stalls for good
        track.poses.append(pose)
        track.deltas.append(delta)
        track.final_errors.append(r.final_error)
        track.iterations.append(r.num_iterations)
        track.converged.append(bool(r.converged))
        track.gated.append(bool(bad))
        track.map_rows.append(table.size())
        track.frame_ms.append(1e3 * (time.perf_counter() - t0))
        if on_frame:
            on_frame(k, table, guess, r)
    return track


def drift(frames, poses, max_range=100.0, orc=None):
    """-> dict: frame-to-frame and scan-to-map ATE rms [m], ICP passes and gated registrations of each, with the oracle"""
    from lidar_slam_from_scratch_amd import odometry
    if orc is None:
        from oracle import oracle as orc
    f2f = odometry.run_odometry(frames, lambda s, t, it, tol: orc.icp_point_to_plane(s, t, max_iterations=it, tolerance=tol,
                                                                                     nthreads=4))
    s2m = run_local_map(frames, oracle_align(orc), max_range=max_range)
    return dict(f2f_ate=odometry.absolute_trajectory_error(f2f, poses), s2m_ate=odometry.absolute_trajectory_error(s2m, poses),
                f2f_passes=int(sum(f2f.iterations)), s2m_passes=int(sum(s2m.iterations)),
                f2f_gated=int(sum(f2f.gated)), s2m_gated=int(sum(s2m.gated)), map_rows=s2m.map_rows[-1])


def drive(n, beams, azimuths, **kw):
    from lidar_slam_from_scratch_amd import synth
    return ([synth.lidar_frame(f, beams=beams, azimuths=azimuths, **kw) for f in range(n)],
            [synth.lidar_pose(f, **kw) for f in range(n)])


def main():
    from lidar_slam_from_scratch_amd import synth
    cases = [("beams=32, azimuths=900, 12 frames", (12, 32, 900), {}), ("beams=16, azimuths=600, 12 frames", (12, 16, 600), {})]
    if "--long" in sys.argv:
        cases.append(("DRIVE_200, 64 x 1800, 40 frames", (40, 64, 1800), synth.DRIVE_200))
    for name, args, kw in cases:
        frames, poses = drive(*args, **kw)
        d = drift(frames, poses)
        print("%-36s f2f %.4f m  s2m %.4f m  passes %d / %d  gated %d / %d  map rows %d"
              % (name, d["f2f_ate"], d["s2m_ate"], d["f2f_passes"], d["s2m_passes"], d["f2f_gated"], d["s2m_gated"], d["map_rows"]))


if __name__ == "__main__":
    main()
