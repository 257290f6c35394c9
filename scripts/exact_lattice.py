"""scripts/exact_lattice.py -- registration fixtures whose normal equations are exact integers (CPU only), for
tests/test_exact_fixture.py and tests/test_gpu_exact_sums.py.

Every product and every partial sum of a pass is exactly representable on these clouds, so ANY order of additions gives
the same bits: the 28 (29, 30) sums of a pass can be held to an integer reference bit for bit, whichever reduction tree
formed them, and the 6 x 6 solve then starts from bit-equal inputs on every side.

Target.  Axis-aligned SIDE x SIDE lattice patches of spacing H = 1/4 whose origins are multiples of 1/8, one per cell of
a 3 x 3 x 3 grid of pitch 16: two patches are at least 6 m apart, a 20-neighbour search reaches 1.5 m (a corner's
quarter disc of 20 lattice points), so no neighbourhood mixes patches and every row's normal is its patch's axis.  Patch
j is normal to axis j mod 3.  The rows are shuffled by a seeded permutation.

Source.  src[i] = tgt[i mod m] + off[(i + i // m) mod K] for a table `off` of K offsets (or off[(2 patch + half) mod K]
of the row's half patch with per_patch=True), every component a multiple of 1/64 and shorter than H / 2: row i's nearest
target is row i mod m and no other (the nearest other lattice point is H - |o| > |o| away along an in-plane axis), for
any n.  (i + i // m, not i // m alone: a source of fewer than m rows meets the whole table too, and a second round over
the target gives each row another offset.)

Reference.  Coordinates times UNIT = 64 are integers below 2^12; integer_sums forms p x n, b and the weighted products
in int64 and converts each sum once.  It asserts that the sum of the ABSOLUTE values of a column's terms stays below
2^53 in the column's unit: then every term and every partial sum, in any order, is a representable number.

Variants (offset tables below):
  plain   PLAIN_OFFSETS
  gate    g = 5/64: rows at |q - p|^2 == g^2 exactly (offsets (3, 4, 0)/64 and their kin: kept), rows inside, and rows
          whose source coordinate is the next representable number further out (d2 > g2 by thousands of ulps: dropped)
  Huber   k = 1/64, offsets with components in {0, +-k, +-2k, +-4k}: b is minus the component along the row's normal, so
          the weights are 1, 1, 1/2, 1/4, all exact, like every w * J
  Geman-McClure  k = 1/64, components in {0, +-k}: s = k^2, t = s + b^2 is k^2 or 2 k^2, r = s / t is 1 or 1/2 and
          w = r^2 is 1 or 1/4, each step exact (tests/test_exact_fixture.py confirms it with robust_icp_ref.weights).  No
          other |b| has an exact r: k^2 / (k^2 + b^2) is a power of two only for b = 0 and b = +-k.
  step    offsets that differ from half patch to half patch, so that one iteration's solution rotates
  cyclic_step  the same on target(cyclic=True) with n = m: target, source and hence JtJ are invariant under the cyclic
          permutation of the axes, so the three rotation diagonals of JtJ are tied and so are the three translation
          diagonals: which of equal diagonals the solve takes as its pivot decides the order of its operations

hand_made_systems(): (source, target, "normals") triples for solve_point_to_plane with small-integer or dyadic data."""
import numpy as np

H = 0.25
SIDE = 40
UNIT = 64                      # every fixture coordinate is a multiple of 1 / UNIT
PITCH = 16.0
GATE = 5.0 / 64.0
HUBER_K = 1.0 / 64.0
GM_K = 1.0 / 64.0

_F = 1.0 / 64.0
PLAIN_OFFSETS = np.array([(4, -2, 6), (-6, 4, 2), (2, 6, -4), (0, -6, 6), (-4, 0, -2)]) * _F
# kept at the gate (3-4-5 triples, |o| = 5/64), kept inside, and three that nextafter() pushes outside
GATE_OFFSETS = np.array([(3, 4, 0), (-4, 0, 3), (0, -3, -4), (4, -3, 0), (2, 2, 1), (0, 0, 0), (-1, 3, 2),
                         (3, 4, 0), (0, 4, -3), (-3, 0, -4)]) * _F
GATE_OUTSIDE = np.array([0, 0, 0, 0, 0, 0, 0, 1, 1, 1], dtype=bool)
HUBER_OFFSETS = np.array([(0, 1, -2), (4, 0, 1), (-1, 2, 4), (2, -4, 0), (-4, -1, 2), (1, 4, -1), (-2, 0, -4),
                          (0, 0, 0)]) * _F
GM_OFFSETS = np.array([(0, 1, -1), (1, 0, 1), (-1, -1, 0), (0, 0, 0), (1, -1, 1)]) * _F
# (per half patch of the cyclic target: patch j's pair is patch 0's with its axes rolled j times -- p x n, hence JtJ, looks at
# the in-plane components alone -- and then a component of its own along the normal, so that Jtb has no symmetry)
CYCLIC_STEP_OFFSETS = np.array([np.roll(o, j) for j in range(3) for o in ((0, -2, 6), (0, 5, 1))]) * _F
CYCLIC_STEP_OFFSETS[np.arange(6), np.arange(6) // 2] = np.array([4, -3, 2, 5, -6, 1]) * _F
STEP_PATCH_OFFSETS = np.array([(4, -2, 6), (-6, 5, 2), (2, 6, -5), (1, -6, 3), (-4, 0, -2), (6, 3, -1), (-2, -5, 4),
                               (5, 1, -6), (-3, 4, 1)]) * _F


class Target:
    """pts (m x 3), axis (m: the normal's axis), patch (m: the patch a row belongs to), half (m: 0 or 1, the half of its
    patch along the first in-plane axis)"""


CYCLIC_ORIGIN = np.array([20.0, -4.0, -6.0])


def target(patches=3, side=SIDE, seed=1, cyclic=False):
    """cyclic: three patches that are the images of one under (x, y, z) -> (z, x, y)"""
    if not 1 <= patches <= 27 or (cyclic and patches != 3):
        raise ValueError("1 to 27 patches, three of them when cyclic")
    u, v = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    u, v = u.ravel() * H, v.ravel() * H
    pts, axis, patch, half = [], [], [], []
    for j in range(patches):
        cell = np.array(np.unravel_index(j, (3, 3, 3)), dtype=np.float64) - 1.0
        origin = cell * PITCH + np.array([j % 4, (j // 2) % 4, (j // 3) % 4]) / 8.0
        if cyclic:
            origin = np.roll(CYCLIC_ORIGIN, j)
        a = j % 3
        p = np.tile(origin, (side * side, 1))
        p[:, (a + 1) % 3] += u
        p[:, (a + 2) % 3] += v
        pts.append(p)
        axis.append(np.full(side * side, a))
        patch.append(np.full(side * side, j))
        half.append((u >= side * H / 2).astype(np.int64))
    order = np.random.default_rng(seed).permutation(patches * side * side)
    t = Target()
    t.pts = np.ascontiguousarray(np.concatenate(pts)[order])
    t.axis = np.concatenate(axis)[order]
    t.patch = np.concatenate(patch)[order]
    t.half = np.concatenate(half)[order]
    return t


class Source:
    """pts (n x 3), match (n: the target row each source row was made from), off (n x 3: the offset it was given, before
    any nextafter), outside (n: pushed one representable number beyond the gate)"""


def source(tgt, n, offsets, per_patch=False, outside=None):
    m = tgt.pts.shape[0]
    i = np.arange(n)
    s = Source()
    s.match = i % m
    which = (2 * tgt.patch[s.match] + tgt.half[s.match]) % len(offsets) if per_patch else (i + i // m) % len(offsets)
    s.off = np.asarray(offsets)[which]
    assert np.abs(s.off).max() < H / 2
    s.pts = tgt.pts[s.match] + s.off
    assert np.array_equal(s.pts - tgt.pts[s.match], s.off)           # the sum was exact
    s.outside = np.zeros(n, dtype=bool) if outside is None else np.asarray(outside)[which]
    if s.outside.any():
        # the first non-zero component of the offset, one representable source coordinate further from the target
        c = np.argmax(s.off != 0.0, axis=1)
        rows = np.nonzero(s.outside)[0]
        away = np.where(s.off[rows, c[rows]] > 0, np.inf, -np.inf)
        s.pts[rows, c[rows]] = np.nextafter(s.pts[rows, c[rows]], away)
    s.pts = np.ascontiguousarray(s.pts)
    return s


def axis_normals(axis):
    n = np.zeros((len(axis), 3))
    n[np.arange(len(axis)), axis] = 1.0
    return n


def _ints(x):
    xi = np.rint(x * UNIT)
    assert np.array_equal(xi, x * UNIT), "a coordinate is not a multiple of 1 / UNIT"
    return xi.astype(np.int64)


def huber_w4(off_n, k=HUBER_K):
    """4 w of Huber's weight for residuals b = -off_n among {0, +-k, +-2k, +-4k}"""
    a = np.rint(np.abs(off_n) / k).astype(np.int64)
    assert np.isin(a, (0, 1, 2, 4)).all()
    return np.where(a <= 1, 4, 4 // np.maximum(a, 1))


def gm_w4(off_n, k=GM_K):
    """4 w of Geman-McClure's weight for residuals among {0, +-k}"""
    a = np.rint(np.abs(off_n) / k).astype(np.int64)
    assert np.isin(a, (0, 1)).all()
    return np.where(a == 0, 4, 1)


class Sums:
    """JtJ (6 x 6), Jtb (6), sum_sq, weight, pairs as floats converted once from integers; largest: the largest sum of
    absolute terms over the columns, in the column's integer unit (asserted below 2^53)"""

    def sums28(self):
        """the oracle's layout: 21 upper-triangle entries row by row, 6 Jtb, sum b^2"""
        return np.array([self.JtJ[r, c] for r in range(6) for c in range(r, 6)] + list(self.Jtb) + [self.sum_sq])


def integer_sums(src_pts, tgt_pts, axis, w4=None, keep=None):
    """The normal equations of the rows `keep` (default all) of a pass that matches src_pts[i] with tgt_pts[i], normal
    axis[i], row weights w4 / 4 (default 1), in integer arithmetic."""
    n = len(src_pts)
    keep = np.ones(n, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    w4 = np.full(n, 4, dtype=np.int64) if w4 is None else np.asarray(w4, dtype=np.int64)
    P, Q = _ints(np.asarray(src_pts)[keep]), _ints(np.asarray(tgt_pts)[keep])
    N = axis_normals(np.asarray(axis)[keep]).astype(np.int64)
    W = w4[keep]
    J = np.concatenate([np.cross(P, N), N], axis=1)                  # columns 0-2 in 1 / UNIT, 3-5 in 1
    power = np.array([1, 1, 1, 0, 0, 0])                             # of UNIT, per column of J
    b = np.sum((Q - P) * N, axis=1)                                  # in 1 / UNIT
    out = Sums()
    out.largest = 0

    def total(terms, unit_power):
        mass = int(np.sum(np.abs(terms)))
        assert mass < 2 ** 53, "the fixture is not exact: a column's absolute terms add up to 2^53 or more"
        out.largest = max(out.largest, mass)
        return int(np.sum(terms)) / float(4 * UNIT ** unit_power)

    out.JtJ = np.zeros((6, 6))
    out.Jtb = np.zeros(6)
    for r in range(6):
        for c in range(r, 6):
            out.JtJ[r, c] = out.JtJ[c, r] = total(W * J[:, r] * J[:, c], power[r] + power[c])
        out.Jtb[r] = total(W * J[:, r] * b, power[r] + 1)
    out.sum_sq = total(W * b * b, 2)
    out.weight = total(W, 0)
    out.pairs = int(keep.sum())
    return out


def variant(kind, tgt, n):
    """-> (Source, keep mask, 4 w per row, Sums) of the variant `kind` (plain, gate, huber, gm, step, cyclic_step) with n
    source rows"""
    if kind == "plain":
        s = source(tgt, n, PLAIN_OFFSETS)
    elif kind == "gate":
        s = source(tgt, n, GATE_OFFSETS, outside=GATE_OUTSIDE)
    elif kind == "huber":
        s = source(tgt, n, HUBER_OFFSETS)
    elif kind == "gm":
        s = source(tgt, n, GM_OFFSETS)
    elif kind == "step":
        s = source(tgt, n, STEP_PATCH_OFFSETS, per_patch=True)
    elif kind == "cyclic_step":
        s = source(tgt, n, CYCLIC_STEP_OFFSETS, per_patch=True)
    else:
        raise ValueError(kind)
    keep = ~s.outside
    off_n = s.off[np.arange(n), tgt.axis[s.match]]
    w4 = huber_w4(off_n) if kind == "huber" else gm_w4(off_n) if kind == "gm" else np.full(n, 4, dtype=np.int64)
    clean = np.where(keep[:, None], s.pts, tgt.pts[s.match])         # (a dropped row's coordinates are not dyadic)
    return s, keep, w4, integer_sums(clean, tgt.pts[s.match], tgt.axis[s.match], w4, keep)


# ---- hand-made 6 x 6 systems ---------------------------------------------------------------------------------------
_BASE = np.array([(1, 2, 3), (-2, 1, 4), (3, -1, 2), (2, 3, -1), (4, -3, 1), (-1, -2, -3), (0, 4, -2)], dtype=np.float64)


def _cyclic(points):
    """every point with normal e_z, and both cyclic images of the pair: all three rotation diagonals of JtJ are tied,
    and so are the three translation diagonals"""
    p, n = [], []
    for k in range(3):
        p.append(np.roll(points, k, axis=1))
        n.append(np.tile(np.roll(np.array([0.0, 0.0, 1.0]), k), (len(points), 1)))
    return np.concatenate(p), np.concatenate(n)


def _with_solution(p, n, x0):
    """targets q = p + n b with b = J x0: the system's least-squares solution is x0 (to rounding)"""
    J = np.concatenate([np.cross(p, n), n], axis=1)
    b = J @ np.asarray(x0, dtype=np.float64)
    return p + n * b[:, None]


def hand_made_systems():
    """name -> (source, target, normals, expect); expect: "oracle" (translation column bit-equal to the oracle's,
    rotation within the sin / cos bound), "identity" (exactly the identity) or "nan" (NaN at the oracle's positions).
    All products and sums of these systems are exact (small integers times one power of two per system), except where a
    row holds a NaN."""
    out = {}
    p, n = _cyclic(_BASE)
    x_small = np.array([2, -1, 3, 8, -4, 2]) / 64.0
    out["full_rank_ties"] = (p, _with_solution(p, n, x_small), n, "oracle")
    u, v = np.meshgrid(np.arange(-2, 3), np.arange(-2, 3), indexing="ij")
    patch = np.stack([u.ravel(), v.ravel(), np.full(25, 3)], axis=1).astype(np.float64)
    nz = np.tile([0.0, 0.0, 1.0], (25, 1))
    out["rank3_one_patch"] = (patch, _with_solution(patch, nz, np.array([1, -2, 0, 0, 0, 4]) / 32.0), nz, "oracle")
    line = np.stack([np.arange(1, 8), np.zeros(7), np.zeros(7)], axis=1).astype(np.float64)
    nl = np.tile([0.0, 0.0, 1.0], (7, 1))
    out["rank2_line"] = (line, _with_solution(line, nl, np.array([0, 3, 0, 0, 0, -2]) / 16.0), nl, "oracle")
    one = np.array([[1.0, 2.0, 3.0]])
    out["rank1_one_row"] = (one, one + np.array([[0.0, 0.0, 0.25]]), np.array([[0.0, 0.0, 1.0]]), "oracle")
    out["zero_normals"] = (p, p + 0.125, np.zeros_like(n), "identity")
    # The pseudo-inverse rule (|D_i| <= DBL_MIN -> x_i = 0).  Points times 8 keep the rotation block's entries multiples of
    # 2^-1074.  Normals of 2^-540: every pivot is subnormal (the translation diagonals underflow to zero), while residuals
    # of 2^530 keep Jtb normal and non-zero -- the rule gives x = 0, the identity, where a division would give 2^530 and
    # more.  Normals of 2^-513: the rotation pivots are normal numbers, the translation pivots (7 * 2^-1026 on the
    # diagonal) are not, and Jtb is subnormal but exact -- the rule solves the rotation and zeroes the translation.
    x_rule = np.array([2, -1, 3, 8, -4, 2]) / 64.0
    q = _with_solution(8.0 * p, n, x_rule)
    out["normals_2^-540"] = (8.0 * p, 8.0 * p + (q - 8.0 * p) * 2.0 ** 530, n * 2.0 ** -540, "oracle")
    out["normals_2^-513"] = (8.0 * p, q, n * 2.0 ** -513, "oracle")
    bad = p.copy()
    bad[4, 0] = np.nan
    out["nan_row"] = (bad, _with_solution(p, n, x_small), n, "nan")
    # rotation norms on either side of pi / 4 = 0.785398...: 0.784528 and 0.786231
    out["under_pi_4"] = (p, _with_solution(p, n, np.array([128, 128, 87, 16, -8, 4]) / 256.0), n, "oracle")
    out["over_pi_4"] = (p, _with_solution(p, n, np.array([128, 128, 88, 16, -8, 4]) / 256.0), n, "oracle")
    out["below_1e-10"] = (p, _with_solution(p, n, np.array([4, -2, 1, 8, -16, 4]) * 2.0 ** -42), n, "oracle")
    return out


def ldlt6_solve(M, rhs, d_min):
    """oracle/icp_oracle.c's ldlt6_solve (Eigen's LDLT: pivot on the first largest |diagonal|, the first-pivot bail-out,
    inner sums in index order) with the pseudo-inverse's threshold as a parameter: x_i = 0 where |D_i| <= d_min.
    sys.float_info.min is the rule; 0.0 is a plain division, what the rule is told apart from."""
    M = np.array(M, dtype=np.float64)
    n = 6
    tr = list(range(n))
    with np.errstate(all="ignore"):
        for k in range(n):
            big = k
            for i in range(k + 1, n):
                if abs(M[i, i]) > abs(M[big, big]):
                    big = i
            tr[k] = big
            if big != k:
                for j in range(k):
                    M[k, j], M[big, j] = M[big, j], M[k, j]
                for i in range(big + 1, n):
                    M[i, k], M[i, big] = M[i, big], M[i, k]
                M[k, k], M[big, big] = M[big, big], M[k, k]
                for i in range(k + 1, big):
                    M[i, k], M[big, i] = M[big, i], M[i, k]
            if k > 0:
                temp = [M[j, j] * M[k, j] for j in range(k)]
                acc = 0.0
                for j in range(k):
                    acc += M[k, j] * temp[j]
                M[k, k] -= acc
                for i in range(k + 1, n):
                    sacc = 0.0
                    for j in range(k):
                        sacc += M[i, j] * temp[j]
                    M[i, k] -= sacc
            valid = abs(M[k, k]) > 0.0
            if k == 0 and not valid:
                tr = list(range(n))
                break
            if valid:
                for i in range(k + 1, n):
                    M[i, k] /= M[k, k]
        x = [float(v) for v in rhs]
        for k in range(n):
            x[k], x[tr[k]] = x[tr[k]], x[k]
        for i in range(n):
            sacc = 0.0
            for j in range(i):
                sacc += M[i, j] * x[j]
            x[i] -= sacc
        for i in range(n):
            x[i] = x[i] / M[i, i] if abs(M[i, i]) > d_min else 0.0
        for i in range(n - 1, -1, -1):
            sacc = 0.0
            for j in range(i + 1, n):
                sacc += M[j, i] * x[j]
            x[i] -= sacc
        for k in range(n - 1, -1, -1):
            x[k], x[tr[k]] = x[tr[k]], x[k]
    return np.array(x), np.diag(M).copy()


def sums_to_system(sums28):
    """the oracle's 28 sums -> (6 x 6 matrix, right-hand side)"""
    M = np.zeros((6, 6))
    o = 0
    for r in range(6):
        for c in range(r, 6):
            M[r, c] = M[c, r] = sums28[o]
            o += 1
    return M, np.array(sums28[21:27])


def rotation_norm(src, tgt, nrm):
    """|x[0:3]| of the least-squares solution, from numpy (which branch of the step a system takes)"""
    J = np.concatenate([np.cross(src, nrm), nrm], axis=1)
    b = np.sum((tgt - src) * nrm, axis=1)
    x = np.linalg.lstsq(J, b, rcond=None)[0]
    return float(np.linalg.norm(x[:3]))


if __name__ == "__main__":
    for patches, n in ((3, 4800), (18, 131089)):
        t = target(patches)
        for kind in ("plain", "gate", "huber", "gm", "step"):
            s, keep, w4, sums = variant(kind, t, n)
            print("%-6s target %6d source %6d kept %6d weight %10.2f largest column mass 2^%.1f"
                  % (kind, len(t.pts), n, sums.pairs, sums.weight, np.log2(max(sums.largest, 1))))
