"""scripts/gicp_ref.py -- the CPU restatement of plane-to-plane (generalized) ICP that
tests/test_gicp_header.py, tests/test_gicp_reference.py and tests/test_gpu_gicp.py hold the library to.

Both clouds carry a local surface model: the plane-regularised covariance U diag(1, 1, epsilon) U^T of a row with unit
normal n is I - (1 - epsilon) n n^T, so the normals are all either side needs and no eigendecomposition is run.

Per pass, for row i of the moved source `cur` with nearest target j (`found`: the row has a neighbour), in unfused fp64
and in this order:

    R    = rotation block of IcpState::total as the pass finds it (total[0..2], [4..6], [8..10])
    s    = normal of source row i, estimated ONCE per call on the source as the caller gave it
           (before initial_transform; k = options.normal_k; the normals launch_normals gives)
    m_a  = (R[a][0]*s0 + R[a][1]*s1) + R[a][2]*s2
    n    = normal of target j;  p = cur_i;  e = q_j - p;  d2 = (e0*e0 + e1*e1) + e2*e2
    kept iff found && d2 <= g2      (g2 = max_distance^2, or DBL_MAX when max_distance == 0)
    c = 1 - epsilon, kappa = 2*epsilon            (formed once on the host)
    S_ab = (a==b ? 2.0 : 0.0) - c*(n_a*n_b + m_a*m_b)          for a <= b
    C00 = S11*S22 - S12*S12;  C01 = S02*S12 - S01*S22;  C02 = S01*S12 - S02*S11
    C11 = S00*S22 - S02*S02;  C12 = S01*S02 - S00*S12;  C22 = S00*S11 - S01*S01
    det = (S00*C00 + S01*C01) + S02*C02;  r = 1.0/det;  M_ab = C_ab*r      (one division per kept row)
    u_a = (M_a0*e0 + M_a1*e1) + M_a2*e2
    A   = [ -[p]x | I ]:  A0 = (0, p2, -p1, 1,0,0), A1 = (-p2, 0, p0, 0,1,0), A2 = (p1, -p0, 0, 0,0,1)
    B   = [p]x M (rows 0..2 against columns 3..5 of A^T M A; M_ab = M_ba):
          B0c = p1*M2c - p2*M1c;  B1c = p2*M0c - p0*M2c;  B2c = p0*M1c - p1*M0c
    G   = B (-[p]x) (rows and columns 0..2), for r <= c only:
          Gr0 = Br2*p1 - Br1*p2;  Gr1 = Br0*p2 - Br2*p0;  Gr2 = Br1*p0 - Br0*p1
    v   = p x u:  v0 = p1*u2 - p2*u1;  v1 = p2*u0 - p0*u2;  v2 = p0*u1 - p1*u0

Columns of a kept row (the gated call's layout; a dropped row adds nothing):

    0..20   the upper triangle of A^T M A, row by row:
            G00 G01 G02 B00 B01 B02 | G11 G12 B10 B11 B12 | G22 B20 B21 B22 | M00 M01 M02 | M11 M12 | M22
    21..26  A^T u = v0 v1 v2 u0 u1 u2
    27      kappa * ((e0*u0 + e1*u1) + e2*u2)
    28      1.0

The step solves H x = g with H = sum A^T M A and g = sum A^T M e; in the point-to-plane limit M = n n^T these are J J^T
and J b, so the solve is the oracle's (solve_from_sums).  error = sqrt(sums[27] / sums[28]); kappa makes it read in
metres: with parallel normals kappa e^T M e = (e.n)^2 + epsilon * (tangential)^2.  epsilon = 1 gives S = 2 I and
M = I / 2 exactly: point-to-point ICP.  A pass that keeps no row ends the call as gated_icp's does.  Step, composition,
post-loop entry and the history invariants are icp.hpp:157-258 as oracle/icp_oracle.c restates it.

The sums are formed in numpy, row after row in index order (a cumulative sum, not numpy's pairwise one).

    gicp_row_columns(p, q, n, m, c, kappa)   the 29 columns of every row given (all kept)
    rotate_normals(total, s)                 m of every row
    gicp_sums(p, q, n, m, c, kappa)          their sums, row after row
    gicp_icp(source, target, epsilon, max_distance=0.0, ...)
    gicp_align(epsilon, max_distance)        gicp_icp as run_odometry's `align` (robust_icp_ref.odometry_ate)
    GicpOracleBackend(epsilon, max_distance) gicp_icp behind loop_yaw_ref.YawLoopClosureDetector's backend interface

The library's small form (ICPMI_GICP_FORM_SMALL: k_icp_small_gicp) forms these rows word for word and adds them in another
order; it is held to this restatement within the same bounds as the general path.

Run as a script it prints DESIGN 7.16's accuracy table: point-to-plane, Huber 0.1 m and plane-to-plane on the C2 pair, on
the cars pair behind 2 m and over frames 0..11 of the default drive, then the L12 loop-verification row: Huber 0.1 m and
plane-to-plane behind the 2 m gate."""
import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gated_icp_ref as gr  # noqa: E402
import loop_yaw_ref as yr  # noqa: E402

DBL_MAX = sys.float_info.max
EPSILON_DEFAULT = 1e-3        # ICPMI_GICP_EPSILON_DEFAULT
NORMAL_K = 20                 # icpmi_options::normal_k's default (icp.hpp:170)


def rotate_normals(total, s):
    """m of every row of s: the source normals in the target frame, under the rotation block of `total`"""
    R = np.asarray(total, dtype=np.float64).reshape(4, 4)
    m = np.empty_like(s)
    for a in range(3):
        m[:, a] = (R[a, 0] * s[:, 0] + R[a, 1] * s[:, 1]) + R[a, 2] * s[:, 2]
    return m


def gicp_row_columns(p, q, n, m, c, kappa):
    """the 29 columns of every row (N x 3 arrays: moved source rows, matched targets, their normals, the rotated source
    normals), in the contract's order of operations -> N x 29"""
    p0, p1, p2 = p[:, 0], p[:, 1], p[:, 2]
    n0, n1, n2 = n[:, 0], n[:, 1], n[:, 2]
    m0, m1, m2 = m[:, 0], m[:, 1], m[:, 2]
    e = q - p
    e0, e1, e2 = e[:, 0], e[:, 1], e[:, 2]
    S00 = 2.0 - c * (n0 * n0 + m0 * m0)
    S01 = 0.0 - c * (n0 * n1 + m0 * m1)
    S02 = 0.0 - c * (n0 * n2 + m0 * m2)
    S11 = 2.0 - c * (n1 * n1 + m1 * m1)
    S12 = 0.0 - c * (n1 * n2 + m1 * m2)
    S22 = 2.0 - c * (n2 * n2 + m2 * m2)
    C00 = S11 * S22 - S12 * S12
    C01 = S02 * S12 - S01 * S22
    C02 = S01 * S12 - S02 * S11
    C11 = S00 * S22 - S02 * S02
    C12 = S01 * S02 - S00 * S12
    C22 = S00 * S11 - S01 * S01
    det = (S00 * C00 + S01 * C01) + S02 * C02
    r = 1.0 / det
    M00, M01, M02, M11, M12, M22 = C00 * r, C01 * r, C02 * r, C11 * r, C12 * r, C22 * r
    u0 = (M00 * e0 + M01 * e1) + M02 * e2
    u1 = (M01 * e0 + M11 * e1) + M12 * e2
    u2 = (M02 * e0 + M12 * e1) + M22 * e2
    B00, B01, B02 = p1 * M02 - p2 * M01, p1 * M12 - p2 * M11, p1 * M22 - p2 * M12
    B10, B11, B12 = p2 * M00 - p0 * M02, p2 * M01 - p0 * M12, p2 * M02 - p0 * M22
    B20, B21, B22 = p0 * M01 - p1 * M00, p0 * M11 - p1 * M01, p0 * M12 - p1 * M02
    cols = np.empty((p.shape[0], 29))
    cols[:, 0] = B02 * p1 - B01 * p2
    cols[:, 1] = B00 * p2 - B02 * p0
    cols[:, 2] = B01 * p0 - B00 * p1
    cols[:, 3], cols[:, 4], cols[:, 5] = B00, B01, B02
    cols[:, 6] = B10 * p2 - B12 * p0
    cols[:, 7] = B11 * p0 - B10 * p1
    cols[:, 8], cols[:, 9], cols[:, 10] = B10, B11, B12
    cols[:, 11] = B21 * p0 - B20 * p1
    cols[:, 12], cols[:, 13], cols[:, 14] = B20, B21, B22
    cols[:, 15], cols[:, 16], cols[:, 17] = M00, M01, M02
    cols[:, 18], cols[:, 19] = M11, M12
    cols[:, 20] = M22
    cols[:, 21] = p1 * u2 - p2 * u1
    cols[:, 22] = p2 * u0 - p0 * u2
    cols[:, 23] = p0 * u1 - p1 * u0
    cols[:, 24], cols[:, 25], cols[:, 26] = u0, u1, u2
    cols[:, 27] = kappa * ((e0 * u0 + e1 * u1) + e2 * u2)
    cols[:, 28] = 1.0
    return cols


def gicp_sums(p, q, n, m, c, kappa):
    """the 29 sums over the rows given (all kept), each added row after row in index order"""
    return np.cumsum(gicp_row_columns(p, q, n, m, c, kappa), axis=0)[-1]   # (sequential, unlike np.sum)


def normal_matrix(sums):
    """-> (H 6 x 6, g) of 29 sums: the layout icpmi_last_normal_matrix hands over"""
    H = np.zeros((6, 6))
    o = 0
    for a in range(6):
        for b in range(a, 6):
            H[a, b] = H[b, a] = sums[o]
            o += 1
    return H, np.array(sums[21:27])


def check_rule(epsilon, max_distance):
    if not (math.isfinite(epsilon) and 0.0 < epsilon <= 1.0):
        raise ValueError("epsilon must be finite with 0 < epsilon <= 1")
    if max_distance != 0.0 and not (max_distance > 0.0 and math.isfinite(max_distance)):
        raise ValueError("max_distance must be 0 or finite and > 0")


class GicpResult:
    """ICPResult's fields (types.hpp:155-164) + pairs and sums (of the pass that produced final_error) + stop_margin (the
    smallest | |prev - error| - tolerance | over the loop's passes: how far the iteration count is from hanging on
    rounding) + gate_margin (the smallest |d2 - g2| over every row of every pass; inf without a gate)"""


def gicp_icp(source, target, epsilon=EPSILON_DEFAULT, max_distance=0.0, max_iterations=50, tolerance=1e-6, min_error=1e-9,
             initial_transform=None, orc=None, normals=None, tree=None, source_normals=None):
    """-> GicpResult.  normals / tree: the target's, source_normals: the source's, if the caller has them already."""
    if orc is None:
        from oracle import oracle as orc
    check_rule(epsilon, max_distance)
    src = np.ascontiguousarray(source, dtype=np.float64)
    tgt = np.ascontiguousarray(target, dtype=np.float64)
    gated = max_distance != 0.0
    g2 = float(max_distance) * float(max_distance) if gated else DBL_MAX
    c, kappa = 1.0 - float(epsilon), 2.0 * float(epsilon)
    snrm = source_normals if source_normals is not None else orc.estimate_normals(src, orc.KDTree(src), NORMAL_K)
    tree = tree or orc.KDTree(tgt)                                   # icp.hpp:166
    nrm = normals if normals is not None else orc.estimate_normals(tgt, tree, NORMAL_K)   # :169-171
    T0 = np.eye(4) if initial_transform is None else np.array(initial_transform, dtype=np.float64).reshape(4, 4)
    cur = gr.apply_rt(T0, src)                                       # :174-176
    total = T0.copy()                                                # :178
    prev = DBL_MAX                                                   # :179
    hist, converged = [], False
    gate_margin, stop_margin = math.inf, math.inf

    def one_pass():
        """-> the 29 sums, or None when no row is kept"""
        nonlocal gate_margin
        idx, _ = tree.nearest_batch(cur)
        found = (idx >= 0) & (idx < tgt.shape[0])
        j = np.where(found, idx, 0)
        e = tgt[j] - cur
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            keep = found & (d2 <= g2)                                # (false for a NaN, and for +Inf against DBL_MAX)
            fin = np.isfinite(d2)
            if gated and fin.any():
                gate_margin = min(gate_margin, float(np.min(np.abs(d2[fin] - g2))))
        if not keep.any():
            return None
        m = rotate_normals(total, snrm[keep])
        return gicp_sums(cur[keep], tgt[j[keep]], nrm[j[keep]], m, c, kappa)

    no_pairs, sums = False, None
    for _ in range(int(max_iterations)):                             # :181
        sums = one_pass()
        if sums is None or not (sums[28] > 0.0):                     # no pairs: a break without convergence
            hist += [math.inf, math.inf]
            no_pairs = True
            break
        error = math.sqrt(sums[27] / sums[28])
        hist.append(error)                                           # :207
        stop_margin = min(stop_margin, abs(abs(prev - error) - tolerance))
        if error < min_error or abs(prev - error) < tolerance:       # :210-217
            converged = True
            break
        delta = orc.solve_from_sums(np.ascontiguousarray(sums[:28]))  # :220
        cur = gr.apply_rt(delta, cur)                                # :225-226
        total = gr.mul44(delta, total)                               # :229
        prev = error                                                 # :231
    if not no_pairs:                                                 # :235-252
        sums = one_pass()
        ok = sums is not None and sums[28] > 0.0
        hist.append(math.sqrt(sums[27] / sums[28]) if ok else math.inf)
    r = GicpResult()
    r.transformation = total
    r.converged = converged
    r.error_history = np.array(hist)
    r.num_iterations = len(hist) - 1                                 # :255
    r.final_error = hist[-1]
    r.pairs = 0 if sums is None else int(sums[28])
    r.sums = sums
    r.stop_margin = stop_margin
    r.gate_margin = gate_margin
    return r


def gicp_align(epsilon=EPSILON_DEFAULT, max_distance=0.0, orc=None):
    """gicp_icp as run_odometry's `align`"""
    return lambda s, t, it, tol: gicp_icp(s, t, epsilon, max_distance, it, tol, orc=orc)


class GicpOracleBackend(yr.OracleBackend):
    """gicp_icp behind YawLoopClosureDetector's backend interface (robust_icp_ref.RobustOracleBackend's shape).  Every
    verification is kept in `runs`, in call order; run_of(closure) is the one a closure came from (the detector hands its
    transform array on as it is).  A cloud's tree and normals are formed once and kept by identity: as a target's, and
    -- the same normals -- as a source's."""

    def __init__(self, epsilon=EPSILON_DEFAULT, max_distance=0.0, orc=None):
        super().__init__(orc)
        check_rule(float(epsilon), float(max_distance))
        self.epsilon, self.max_distance = float(epsilon), float(max_distance)
        self.runs = []
        self._normals = {}                                            # per cloud (by identity): (cloud, tree, normals)

    def _cloud(self, c):
        key = id(c)
        if key not in self._normals:
            tree = self.orc.KDTree(c)
            self._normals[key] = (c, tree, self.orc.estimate_normals(c, tree, NORMAL_K))
        return self._normals[key]

    def align(self, s, t, max_iterations, tolerance, *, initial_transform=None):
        _, _stree, snrm = self._cloud(s)
        _, tree, nrm = self._cloud(t)
        r = gicp_icp(s, t, self.epsilon, self.max_distance, max_iterations, tolerance, 1e-9, initial_transform, orc=self.orc,
                     normals=nrm, tree=tree, source_normals=snrm)
        self.iterations.append(r.num_iterations)
        self.runs.append(r)
        return r

    def run_of(self, closure):
        for r in self.runs:
            if r.transformation is closure.transform:
                return r
        raise KeyError("not a closure of this backend")

    def min_margins(self):
        """-> (stopping margin, gate margin) over every verification"""
        return (min((r.stop_margin for r in self.runs), default=math.inf),
                min((r.gate_margin for r in self.runs), default=math.inf))


def l12_run(backend):
    """the L12 drive (gated_icp_ref.l12_scans, l12_config) through `backend` -> (closures, worst error from truth, m)"""
    import robust_icp_ref as rr
    poses, labels, clouds = gr.l12_scans()
    found = gr.run_detector(yr.YawLoopClosureDetector(backend, gr.l12_config()), clouds, labels)
    return found, rr.l12_worst(found, poses, labels)


def subsample_pair(n_src=1001, n_tgt=1500, seed=7):
    """-> (source, target, truth): a seeded subsample of synth.c2_lidar_pair(), rows in index order"""
    from lidar_slam_from_scratch_amd import synth
    s, t, T = synth.c2_lidar_pair()
    rng = np.random.default_rng(seed)
    si = np.sort(rng.choice(s.shape[0], n_src, replace=False))
    ti = np.sort(rng.choice(t.shape[0], n_tgt, replace=False))
    return np.ascontiguousarray(s[si]), np.ascontiguousarray(t[ti]), T


FIXTURE_GATE = 3.0            # the subsampled pairs' gate, metres
CARS_GATE = 2.0


def gpu_fixtures():
    """name -> dict(source, target, start, epsilon, gate, max_iterations): what tests/test_gpu_gicp.py holds the library
    to, and tests/test_gicp_reference.py keeps clear of the stopping test and of the gate.
        sub_1001_1500        a subsample of the C2 pair behind 3 m: four partial rows, the last ragged
        sub_1001_1500_start  the same problem with the source moved by the inverse of a start 1.3 rad away: the source's
                             normals are estimated on the moved rows and R turns them back
        sub_33_700, sub_5_700  one partial row, most lanes idle
        c2, cars             the full pairs (35 partial rows), the cars behind 2 m
        uniform_65537_20000  more rows than 256 x the CU count (a thread sums more than one), three passes"""
    from lidar_slam_from_scratch_amd import synth
    import robust_icp_ref as rr
    out = {}
    s, t, _ = subsample_pair(1001, 1500)
    out["sub_1001_1500"] = dict(source=s, target=t, start=None, epsilon=EPSILON_DEFAULT, gate=FIXTURE_GATE, max_iterations=50)
    start = synth.make_transform((0.3, -0.5, 1.2), (3.0, -2.0, 0.5))
    moved = np.ascontiguousarray(synth.apply_transform(synth.invert_transform(start), s))
    out["sub_1001_1500_start"] = dict(source=moved, target=t, start=start, epsilon=EPSILON_DEFAULT, gate=FIXTURE_GATE, max_iterations=50)
    for n in (33, 5):
        s, t, _ = subsample_pair(n, 700)
        out["sub_%d_700" % n] = dict(source=s, target=t, start=None, epsilon=EPSILON_DEFAULT, gate=0.0, max_iterations=50)
    s, t, _ = synth.c2_lidar_pair()
    out["c2"] = dict(source=s, target=t, start=None, epsilon=EPSILON_DEFAULT, gate=0.0, max_iterations=50)
    s, t, _ = rr.cars_pair()
    out["cars"] = dict(source=s, target=t, start=None, epsilon=EPSILON_DEFAULT, gate=CARS_GATE, max_iterations=50)
    s, t, _ = synth.c3_uniform(65537, seed=61, perm_seed=62)
    out["uniform_65537_20000"] = dict(source=s, target=np.ascontiguousarray(t[:20000]), start=None, epsilon=EPSILON_DEFAULT,
                                      gate=0.0, max_iterations=3)
    return out


def run_fixture(f, orc=None, **kw):
    """gicp_icp on one of gpu_fixtures()' entries"""
    return gicp_icp(f["source"], f["target"], f["epsilon"], f["gate"], f["max_iterations"], 1e-6, 1e-9, f["start"], orc=orc, **kw)


if __name__ == "__main__":
    from oracle import oracle as orc
    from lidar_slam_from_scratch_amd import synth
    import robust_icp_ref as rr

    for name, (s, t, T), gate in (("C2 pair", synth.c2_lidar_pair(), 0.0), ("cars pair, gate 2 m", rr.cars_pair(), 2.0)):
        plain = orc.icp_point_to_plane(s, t)                          # (the oracle has no gate)
        huber = rr.robust_icp(s, t, rr.HUBER, rr.HUBER_SCALE, gate, orc=orc)
        g = gicp_icp(s, t, EPSILON_DEFAULT, gate, orc=orc)
        print("%-20s point-to-plane %.4f m, %d it. | Huber 0.1 %.4f m, %d it. | plane-to-plane %.4f m, %d it., %d pairs, "
              "final error %.4f, margins %.2e / %.2e"
              % (name, rr.truth_error(plain.transformation, T), plain.num_iterations, rr.truth_error(huber.transformation, T),
                 huber.num_iterations, rr.truth_error(g.transformation, T), g.num_iterations, g.pairs, g.final_error,
                 g.stop_margin, g.gate_margin))
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    frames, poses = rr.drive_frames(n)
    for label, align in (("point-to-plane", rr.oracle_align(orc)), ("Huber 0.1", rr.robust_align(rr.HUBER, rr.HUBER_SCALE, orc=orc)),
                         ("plane-to-plane", gicp_align(orc=orc))):
        print("drive 0..%d %-15s ATE rms %.3f m, end %.3f m, %d passes" % ((n - 1, label) + rr.odometry_ate(frames, poses, align)))
    for label, backend in (("Huber 0.1 m, 2 m gate", rr.RobustOracleBackend(rr.HUBER, rr.HUBER_SCALE, gr.L12_GATE, orc)),
                           ("plane-to-plane eps = 1e-3, 2 m gate", GicpOracleBackend(EPSILON_DEFAULT, gr.L12_GATE, orc))):
        found, worst = l12_run(backend)
        stop, gate = backend.min_margins()
        print("L12 %-36s verifications %d, closures %d, worst %.4f m, passes %d, largest final_error %.4f, kept %s, "
              "margins %.2e / %.2e m^2"
              % (label, len(backend.runs), len(found), worst, sum(r.num_iterations for r in backend.runs),
                 max(r.final_error for r in backend.runs), [backend.run_of(c).pairs for c in found], stop, gate))
