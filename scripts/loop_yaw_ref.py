"""scripts/loop_yaw_ref.py -- the CPU restatement of loop-closure detection with Scan Context's yaw guess
that tests/test_loop_yaw_reference.py and tests/test_gpu_loop_yaw.py hold the library to.

ScanContext::distance (core/scan_context.hpp:90-101) takes the minimum of the shifted cosine distance over the 60 column
shifts and drops the shift that attained it.  Kept, that shift is the yaw between the two scans to within half a sector
(3 degrees), and the verification starts from it instead of from the identity (core/loop_closure.hpp:102-109):

    shift_distances(a, b)      the 60 per-shift distances (:121-142), accumulated over (ring, sector) in the reference's
                               order, vectorised over the shift only: min() is oracle.scan_context_distance bit for bit
    distance_shift(a, b)       (the minimum, the SMALLEST shift attaining it): the reference's loop runs upward with a
                               strict <, :94-99; a NaN never wins
    best_shift(a, b)           that shift alone
    shift_transform(shift)     row-major Rz(+shift * 2 pi / 60), the transform source -> target with query = source and
                               candidate = target; shift 0 is the exact identity
    YawLoopClosureDetector     LoopClosureDetector::detect (:66-126), each verification started from its candidate's
                               shift_transform

Sign: a[j] is compared with b[j + shift], so what the query sees at azimuth phi the candidate sees at phi + shift * 6 deg:
the query's points (the source) go into the candidate's frame (the target) by Rz(+shift * 6 deg).  The opposite sign
fails the tests at every heading that is not near 0 or 180 degrees."""
import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

RINGS, SECTORS = 20, 60


def shift_distances(a, b):
    """-> (60,): column_shifted_distance(a, b, shift) for every shift, scan_context.hpp:121-142"""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(RINGS, SECTORS)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(RINGS, SECTORS)
    b2 = np.concatenate([b, b], axis=1)                     # b2[i, j + shift] = b[i, (j + shift) % 60]
    sum_ab, sum_aa, sum_bb = np.zeros(SECTORS), np.zeros(SECTORS), np.zeros(SECTORS)   # :122-124
    for i in range(RINGS):
        for j in range(SECTORS):
            va, vb = a[i, j], b2[i, j:j + SECTORS]          # vb[shift]
            sum_ab = sum_ab + va * vb                       # products rounded, then added: no fused multiply-add
            sum_aa = sum_aa + va * va
            sum_bb = sum_bb + vb * vb
    norm = np.sqrt(sum_aa) * np.sqrt(sum_bb)                # :137
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(norm < 1e-10, 1.0, 1.0 - sum_ab / norm)   # :138-141


def distance_shift(a, b):
    """-> (distance, shift): scan_context.hpp:90-101 with the argmin kept"""
    best, shift = sys.float_info.max, 0                    # :91
    for s, d in enumerate(shift_distances(a, b)):
        if d < best:                                        # :95-98, strict: the first minimum stays; NaN never wins
            best, shift = float(d), s
    return best, shift


def best_shift(a, b):
    return distance_shift(a, b)[1]


def shift_transform(shift):
    """icpmi_sc_shift_transform: row-major Rz(shift * (2 pi / 60))"""
    shift = int(shift)
    if not 0 <= shift < SECTORS:
        raise ValueError("shift outside 0..59")
    angle = shift * (2.0 * math.pi / 60)
    c, s = math.cos(angle), math.sin(angle)
    T = np.eye(4)
    T[0, 0], T[0, 1] = c, 0.0 - s                           # (0.0 - s: +0 at shift 0)
    T[1, 0], T[1, 1] = s, c
    return T


class Closure:
    """LoopClosureResult (loop_closure.hpp:25-31) and the shift its verification started from"""

    def __init__(self, query_frame, match_frame, transform, scan_context_distance, icp_fitness, sector_shift):
        self.query_frame, self.match_frame, self.transform = query_frame, match_frame, transform
        self.scan_context_distance, self.icp_fitness, self.sector_shift = scan_context_distance, icp_fitness, sector_shift


class OracleBackend:
    """the CPU oracle behind loop_closure.LoopClosureDetector's backend interface; counts its verifications"""

    def __init__(self, orc=None):
        if orc is None:
            from oracle import oracle as orc
            orc.build()
        self.orc = orc
        self.iterations = []                                # num_iterations of every align, in call order

    def scan_context(self, cloud):
        return self.orc.scan_context(cloud)

    def distances(self, q, hist):
        return np.array([self.orc.scan_context_distance(q, h) for h in hist])

    def distances_shift(self, q, hist):
        pairs = [distance_shift(q, h) for h in hist]
        return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs], dtype=np.int32)

    def align(self, s, t, max_iterations, tolerance, *, initial_transform=None):
        r = self.orc.icp_point_to_plane(s, t, max_iterations, tolerance, 1e-9, initial_transform=initial_transform)
        self.iterations.append(r.num_iterations)
        return r


class YawLoopClosureDetector:
    """loop_closure.hpp:41-148 with the guess: backend.scan_context(cloud) and
    backend.align(source, target, max_iterations, tolerance, initial_transform=T); the distances are this file's."""

    def __init__(self, backend, config):
        self.backend, self.config = backend, config
        self._descriptors, self._clouds, self._frame_indices = [], [], []

    def add_frame(self, cloud, frame_idx):                  # :54-60
        cloud = np.ascontiguousarray(cloud, dtype=np.float64)
        self._descriptors.append(np.asarray(self.backend.scan_context(cloud)).reshape(RINGS, SECTORS))
        self._clouds.append(cloud)
        self._frame_indices.append(int(frame_idx))

    def size(self):
        return len(self._descriptors)

    def detect(self):                                       # :66-126
        results = []
        if len(self._descriptors) < 2:
            return results
        q = len(self._descriptors) - 1
        candidates = []
        for i in range(q):
            if self._frame_indices[q] - self._frame_indices[i] < self.config.frame_gap:   # :80-82
                continue
            d, s = distance_shift(self._descriptors[q], self._descriptors[i])             # :86, the shift kept
            if d < self.config.sc_distance_threshold:                                     # :87-89
                candidates.append((d, i, s))
        candidates.sort(key=lambda c: c[:2])                # :93 (distance, entry): the shift never enters the order
        verified = 0
        for d, i, s in candidates:                          # :96-123
            if verified >= self.config.max_candidates:
                break
            r = self.backend.align(self._clouds[q], self._clouds[i], 30, 1e-6, initial_transform=shift_transform(s))
            if r.converged and r.final_error < self.config.icp_fitness_threshold:         # :112
                results.append(Closure(self._frame_indices[q], self._frame_indices[i], np.asarray(r.transformation),
                                       d, r.final_error, s))
                verified += 1
        return results


# ------------------------------------------------------------------------------------------------------------ fixed inputs
# The drives the tests and scripts/loop_store_timing.py share: poses (x, y, yaw in degrees) in the synthetic street
# (synth.lidar_frame_at: 32 beams, 900 azimuths, 0.5 m voxels, range noise 0.01, noise seed 1000 + index in the drive),
# with the points within 1e-9 of a sector boundary dropped (there the sector hangs on atan2's last ulp).

def pose(x, y, yaw_deg):
    a = math.radians(yaw_deg)
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    T[0, 3], T[1, 3] = x, y
    return T


def off_sector_boundaries(cloud):
    q = (np.arctan2(cloud[:, 1], cloud[:, 0]) + np.pi) / (2 * np.pi / SECTORS)
    return cloud[np.abs(q - np.round(q)) > 1e-9]


def scans(poses):
    from lidar_slam_from_scratch_amd import synth
    return [off_sector_boundaries(synth.lidar_frame_at(T, 1000 + i, beams=32, azimuths=900)) for i, T in enumerate(poses)]


def truth(poses, query, match):
    """the transform that takes scan `query`'s points into scan `match`'s frame"""
    return np.linalg.inv(poses[match]) @ poses[query]


def r12_reverse_drive():
    """-> (poses, labels): six scans out along a street, six on the way back facing the other way"""
    out = [pose(-20 + 2 * k, 0.3, 2 * k) for k in range(6)]
    back = [pose(-20 + 2 * k, 0.3, 183 - 1.5 * k) for k in range(5, -1, -1)]
    return out + back, list(range(6)) + list(range(100, 106))


def h12_headings():
    """-> (poses, labels): one place at headings 0, 30, .., 300 degrees, then the query at 337"""
    return [pose(-14, 0.3, 30 * k) for k in range(11)] + [pose(-14, 0.3, 337)], list(range(12))


def d78_drive():
    """-> poses: 30 frames out, a turn on the spot over 18 frames, 30 frames back along the same line"""
    xs = [-20 + 0.6 * k for k in range(30)]
    return ([pose(x, 0.3, 0) for x in xs] + [pose(xs[-1], 0.3, 180 * (k + 1) / 19) for k in range(18)]
            + [pose(x, 0.3, 180) for x in reversed(xs)])
