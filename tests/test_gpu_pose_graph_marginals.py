"""Marginal and relative covariances of the optimised poses (icpmi_pose_graph_marginals / _relative_covariance /
_closure_distance; csrc/pose_graph_marginals.h) against the CPU restatement
(scripts/pose_graph_marginals_ref.py), which linearises at the poses the device returned: both sides invert the same
matrix.

Error measure: |dSigma_ab| / sqrt(Sigma_aa Sigma_bb) with the restatement's diagonal.  Allowed per query: the larger of
10 x the spread of the restatement's solves (sparse LU under COLAMD and NATURAL, dense Cholesky; the dense one is left
out above DENSE_MAX poses, where it needs gigabytes: a smaller spread only tightens the bound) and a floor of 8 x the
restatement's own worst error against a 50-digit inverse on the fixture of scripts/make_marginals_case.py.
Order independence, the cached second call and a rebuilt graph are held to bits.

Shapes sit where a kernel can go wrong: no separator at all, a segment with only one separator, a one-node segment,
first and last nodes of segments, separators with their neighbours, reduced systems of 12 .. 372 rows (below, at and
across the 32-row blocks of the column solve) and q up to 40."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pose_graph_info_ref as I  # noqa: E402
import pose_graph_loss_ref as L  # noqa: E402
import pose_graph_marginals_ref as M  # noqa: E402
import pose_graph_ref as R  # noqa: E402
import test_gpu_pose_graph as G  # noqa: E402
from lidar_slam_from_scratch_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

K = G.K
DENSE_MAX = 1500
CASE = np.load(os.path.join(ROOT, "tests", "golden", "pose_graph_marginals_case.npz"))
FLOOR = 8.0 * float(CASE["restatement_error"])


@pytest.fixture(scope="module")
def ctx():
    """Fails loudly (no skip, no fallback) when the HIP library or the device is missing."""
    from lidar_slam_from_scratch_amd import build, capi
    build.build_library()
    c = capi.Context(device=0)
    yield c
    c.close()


def dev_apply(g, ops):
    for op in ops:
        if op[0] == "odom_info":
            g.add_odometry_information(op[1], op[2], op[3], op[4])
        elif op[0] == "loop_info":
            g.add_loop_closure_information(op[1], op[2], op[3], op[4])
        else:
            G.apply(g, [op])


class Case:
    """A graph optimised on the device and the restatement's H at the device's poses."""

    def __init__(self, ctx, ops, loss=None):
        from lidar_slam_from_scratch_amd import pose_graph as pg
        self.dev = pg.PoseGraph(ctx)
        self.ref = I.PoseGraph()
        if loss is not None:
            self.dev.set_loop_loss(*loss)
            self.ref.set_loop_loss(*loss)
        dev_apply(self.dev, ops)
        I.apply(self.ref, ops)
        assert self.dev.optimize()
        self.poses = [np.array(p) for p in self.dev.get_all_poses()]
        self.keys, self.H = M.hessian(self.ref, self.poses)
        self.X = dict(zip(self.keys, self.poses))

    def reference(self, q):
        a = M.joint_marginal(self.H, self.keys, q, "COLAMD")
        spread = M.normalised_error(M.joint_marginal(self.H, self.keys, q, "NATURAL"), a)
        if len(self.keys) <= DENSE_MAX:
            spread = max(spread, M.normalised_error(M.joint_marginal(self.H, self.keys, q, "DENSE"), a))
        return a, max(10.0 * spread, FLOOR)

    def check(self, q, name=""):
        got = self.dev.joint_marginal_covariance(q)
        a, tol = self.reference(q)
        err = M.normalised_error(got, a)
        d = np.sqrt(np.diag(a))
        sym = float(np.max(np.abs(got - got.T) / np.outer(d, d)))
        print("marginals %s q=%d err %.3g asym %.3g tol %.3g" % (name, len(q), err, sym, tol))
        assert got.shape == (6 * len(q), 6 * len(q))
        assert err <= tol, (name, q, err, tol)
        assert sym <= tol, (name, q, sym, tol)
        assert (np.diag(got) > 0.0).all()
        return got


def test_fixture_graph_against_the_50_digit_inverse(ctx):
    """The device on the fixture graph, linearised at its own poses, against the restatement under the usual bound."""
    ops = []
    for k, i, j, z, f in zip(CASE["kind"], CASE["fi"], CASE["fj"], CASE["Z"], CASE["fitness"]):
        ops.append(("prior", int(i), z) if k == 0 else ("odom", int(i), int(j), z, float(f)) if k == 1
                   else ("loop", int(i), int(j), z))
    c = Case(ctx, ops)
    c.check(list(range(20)), "fixture")
    c.check([15, 2], "fixture")


def test_one_pose_with_a_prior(ctx):
    c = Case(ctx, [("prior", 0, synth.make_transform([0.1, -0.2, 0.3], [1, 2, 3]))])
    got = c.check([0], "prior only")
    assert np.abs(np.diag(got) / 1e-6 - 1.0).max() <= FLOOR          # diag(sigma_prior^2), sigma 0.001
    assert np.abs(got - np.diag(np.diag(got))).max() <= FLOOR * 1e-6


def test_chain_of_five(ctx):
    c = Case(ctx, G.chain_ops(5, seed=5))
    for q in ([0], [4], [0, 4], [2, 3], [0, 1, 2, 3, 4]):
        c.check(q, "chain5")


@pytest.mark.parametrize("n", [K - 1, K, K + 1])
def test_chains_around_k(ctx, n):
    """K - 1: no separator; K: a segment with only a right separator (the last node); K + 1: also a one-node segment
    with only a left one."""
    c = Case(ctx, G.chain_ops(n, seed=n))
    c.check([0, n - 1], "chain%d" % n)
    c.check([n // 2, n - 2, n - 1, 1], "chain%d" % n)


@pytest.fixture(scope="module")
def chain193(ctx):
    return Case(ctx, G.chain_ops(3 * K + 1, seed=3 * K + 1))


@pytest.mark.parametrize("q", [
    [0, 62, 64, 126, 128, 190, 192],        # first and last nodes of every segment (192: a one-node segment)
    [62, 63, 64],                           # separator 63 with both neighbours
    [10, 40],                               # two interior nodes of one segment: the W_v[u] term
    [40, 10],
    [10, 100],                              # two interior nodes of different segments
    [100, 127], [64, 63], [191, 192],       # an interior node with its own end separator
    [63, 127, 191],                         # separators only
    [5],
])
def test_chain_of_3k_plus_1(chain193, q):
    chain193.check(q, "chain193")


def test_ring_with_loops_sharing_endpoints(ctx):
    loops = [(m, q) for q in (150, 170, 190) for m in (q - 140, q - 139, q - 137)] + [(63, 127)]
    c = Case(ctx, G.ring_ops(200, 3, loops))
    c.check([10, 150], "ring200")
    c.check([63, 127, 64, 11, 199, 0, 100], "ring200")
    c.check(list(range(0, 200, 5)), "ring200")                     # q = 40


@pytest.mark.parametrize("b,seed", [(2, 21), (5, 22), (6, 23), (11, 24), (16, 25), (17, 26), (62, 30)])
def test_reduced_size_sweep(ctx, b, seed):
    """Reduced systems of 12 .. 372 rows: below, at and across the column solve's 32-row blocks."""
    ops = G.sweep_ops(b, seed)
    seps = sorted(G.separators(ops))
    inner = [k for k in range(62) if k not in seps]
    c = Case(ctx, ops)
    q = [seps[0], seps[-1]] + inner[:1] + inner[-1:]
    c.check(q, "sweep%d" % b)
    c.check(([0, 61, 30, 31, 7, 45, 19] if b < 62 else seps[::9]), "sweep%d" % b)   # q = 7


@pytest.mark.parametrize("q", [1, 2, 4, 7, 40])
def test_query_sizes(chain193, q):
    idx = [int(v) for v in np.random.default_rng(q).choice(193, size=q, replace=False)]
    chain193.check(idx, "q%d" % q)


def test_kitti_shaped_graph(ctx):
    c = Case(ctx, G.kitti_ops())
    c.check([0, 959, 2000, 4540], "kitti")


def test_cauchy_loss_with_a_false_closure(ctx):
    """The rejected edge must not tighten the covariance: the restatement, which applies the loss' weight, decides."""
    ops = L.false_closure_ring(1)
    c = Case(ctx, ops, loss=(L.LOSS_CAUCHY, 3.0))
    w, _ = c.dev.loop_weights()
    assert w[-1] < 1e-2 < w[:-1].min()
    c.check([30, 150, 100, 199], "cauchy")


def test_information_edges(ctx):
    ops, _ = I.anisotropic_ring(1, True)
    c = Case(ctx, ops)
    c.check([0, 90, 199, 63], "info edges")


# ------------------------------------------------------------------------------------------------------------- bits

def _block(S, q, i, j):
    a, b = q.index(i), q.index(j)
    return S[6 * a:6 * a + 6, 6 * b:6 * b + 6]


@pytest.mark.parametrize("i,j", [(10, 40), (62, 63), (5, 150), (63, 127), (192, 0)])
def test_a_block_does_not_depend_on_the_query(chain193, i, j):
    dev = chain193.dev
    qs = [[i, j], [j, i], [100, i, 64, 191, j, 3, 128]]
    S = [dev.joint_marginal_covariance(q) for q in qs]
    for a, b in ((i, i), (i, j), (j, i), (j, j)):
        first = _block(S[0], qs[0], a, b)
        for q, s in zip(qs[1:], S[1:]):
            assert (_block(s, q, a, b) == first).all(), (a, b, q)
    assert (dev.marginal_covariance(i) == _block(S[0], qs[0], i, i)).all()


def test_cached_call_and_rebuilt_graph_give_the_same_bytes(ctx):
    from lidar_slam_from_scratch_amd import pose_graph as pg
    ops = G.ring_ops(200, 3, [(10, 150), (11, 150), (63, 127)])
    q = [0, 10, 63, 64, 150, 199, 77]
    out = []
    for _ in range(2):
        g = pg.PoseGraph(ctx)
        G.apply(g, ops)
        assert g.optimize()
        first = g.joint_marginal_covariance(q)          # factors H
        second = g.joint_marginal_covariance(q)         # cached factor
        assert (first == second).all()
        assert g.optimize()                             # clears the factor; the same optimum, the same bytes
        assert (g.joint_marginal_covariance(q) == first).all()
        out.append(first)
        g.close()
    assert (out[0] == out[1]).all()


# ----------------------------------------------------------------------------------------- relative, distance, errors

def test_relative_covariance_and_closure_distance(ctx):
    ops = L.false_closure_ring(1)
    c = Case(ctx, ops[:-1])
    Se = M.loop_edge_covariance(c.ref.config)
    for (i, j) in ((30, 150), (150, 30), (62, 63), (0, 199)):
        joint, tol = c.reference([i, j])
        want = M.relative_covariance(c.X[i], c.X[j], joint)
        got = c.dev.relative_covariance(i, j)
        # the bound of the joint covariance carried through J: |J| sums 12 entries per row, twice
        d = np.sqrt(np.diag(want))
        Ja = np.abs(np.hstack([R.adjoint(R.inverse(c.X[j]) @ c.X[i]), np.eye(6)]))
        sj = np.sqrt(np.diag(joint))
        bound = tol * (Ja @ np.outer(sj, sj) @ Ja.T)
        err = np.abs(got - want)
        print("relative (%d, %d) err/bound %.3g" % (i, j, float((err / bound).max())))
        assert (err <= bound).all()
        assert (got == got.T).all() and (d > 0).all()
        Z = ops[-1][3]
        d2 = c.dev.closure_distance(i, j, Z, Se)
        ref = M.closure_distance(c.X[i], c.X[j], Z, want, Se)
        # d2 = e^T M^-1 e moves by at most |e|^T M^-1 |dM| M^-1 |e| to first order
        e = R.se3_log(R.inverse(Z) @ (R.inverse(c.X[i]) @ c.X[j]))
        y = np.abs(np.linalg.solve(want + Se, e))
        dtol = 2.0 * float(y @ bound @ y) + 1e-12 * ref
        print("closure distance (%d, %d) %.6g ref %.6g tol %.3g" % (i, j, d2, ref, dtol))
        assert abs(d2 - ref) <= dtol


def test_error_paths(ctx):
    from lidar_slam_from_scratch_amd import capi
    from lidar_slam_from_scratch_amd import pose_graph as pg
    g = pg.PoseGraph(ctx)
    G.apply(g, G.chain_ops(70, seed=70))

    def refused(fn, code=capi.ERR_ARG):
        with pytest.raises(capi.IcpError) as e:
            fn()
        assert e.value.code == code, e.value

    def answers():
        S = g.joint_marginal_covariance([3, 69])
        assert np.isfinite(S).all() and (np.diag(S) > 0).all()
        return S

    refused(lambda: g.joint_marginal_covariance([0]))                  # before any optimize()
    refused(lambda: g.relative_covariance(0, 1))
    assert g.optimize()
    first = answers()
    for bad in ([70], [-1], [3, 3], [5, 9, 5], []):                    # unknown, duplicate, q = 0
        refused(lambda: g.joint_marginal_covariance(bad))
        assert (answers() == first).all()
    lib, h = g._lib, g._h
    idx = (C.c_int64 * 1)(3)
    out = np.zeros((6, 6))
    assert lib.icpmi_pose_graph_marginals(h, None, 1, capi._dp(out)) == capi.ERR_NULL
    assert lib.icpmi_pose_graph_marginals(h, idx, 1, None) == capi.ERR_NULL
    assert lib.icpmi_pose_graph_marginals(None, idx, 1, capi._dp(out)) == capi.ERR_NULL
    assert lib.icpmi_pose_graph_relative_covariance(h, 0, 1, None) == capi.ERR_NULL
    d2 = C.c_double(0.0)
    eye4, eye6 = np.eye(4), np.eye(6)
    assert lib.icpmi_pose_graph_closure_distance(h, 0, 1, None, capi._dp(eye6), C.byref(d2)) == capi.ERR_NULL
    assert lib.icpmi_pose_graph_closure_distance(h, 0, 1, capi._dp(eye4), None, C.byref(d2)) == capi.ERR_NULL
    assert lib.icpmi_pose_graph_closure_distance(h, 0, 1, capi._dp(eye4), capi._dp(eye6), None) == capi.ERR_NULL
    assert (answers() == first).all()
    refused(lambda: g.relative_covariance(4, 4))                       # from == to
    refused(lambda: g.closure_distance(4, 4, eye4, eye6))
    refused(lambda: g.relative_covariance(4, 70))
    assert (answers() == first).all()
    refused(lambda: g.closure_distance(4, 5, eye4, -eye6))             # Sigma_edge not positive definite
    notpd = np.eye(6)
    notpd[0, 1] = notpd[1, 0] = 2.0
    refused(lambda: g.closure_distance(4, 5, eye4, notpd))
    assert g.closure_distance(4, 5, eye4, eye6) >= 0.0
    assert (answers() == first).all()
    g.add_loop_closure(2, 60, np.linalg.inv(g.get_pose(2)) @ g.get_pose(60))   # an add since the last optimize()
    refused(lambda: g.joint_marginal_covariance([3, 69]))
    refused(lambda: g.closure_distance(4, 5, eye4, eye6))
    assert g.optimize()
    answers()
    g.add_prior(5, g.get_pose(5))                                      # a prior leaves `optimized` set but adds a factor
    refused(lambda: g.joint_marginal_covariance([3, 69]))
    assert g.optimize()
    answers()
    g.set_loop_loss(capi.PG_LOSS_CAUCHY, 3.0)
    refused(lambda: g.joint_marginal_covariance([3, 69]))
    assert g.optimize()
    answers()


# ------------------------------------------------------------------------------------------------------------ demo

def test_cpp_demo_gives_the_python_mirrors_bytes(ctx, tmp_path):
    """tests/cpp/pose_graph_marginals_demo.cpp through the C++ mirror header, on the device, against the Python mirror
    on the same graph."""
    from lidar_slam_from_scratch_amd import build
    from lidar_slam_from_scratch_amd import pose_graph as pg
    exe = tmp_path / "pose_graph_marginals_demo"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pose_graph_marginals_demo.cpp"), "-o", str(exe),
                           build.LIB_PATH, "-Wl,-rpath," + os.path.dirname(build.LIB_PATH), "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    n = 80
    step = synth.make_transform([0, 0, 0.05], [1.0, 0.0, 0.0])
    closure = np.linalg.matrix_power(step, 60) @ synth.make_transform([0, 0, 0.002], [0.01, -0.02, 0.0])
    proposed = np.linalg.matrix_power(step, 60) @ synth.make_transform([0, 0, 0.01], [0.1, 0.0, 0.0])
    edge = np.diag([0.005 ** 2] * 3 + [0.025 ** 2] * 3)
    np.concatenate([[float(n)], step.ravel(), closure.ravel(), proposed.ravel(), edge.ravel()]).tofile(tmp_path / "in.f64")
    subprocess.check_call([str(exe), str(tmp_path / "in.f64"), str(tmp_path / "out.f64")], timeout=120)
    o = np.fromfile(tmp_path / "out.f64")
    g = pg.PoseGraph(ctx)
    g.add_prior(0, np.eye(4))
    for k in range(n - 1):
        g.add_odometry_factor(k, k + 1, step, 0.0)
    g.add_loop_closure(5, 65, closure)
    assert g.optimize()
    want = np.concatenate([g.marginal_covariance(40).ravel(), g.joint_marginal_covariance([63, 10]).ravel(),
                           g.relative_covariance(10, 70).ravel(), [g.closure_distance(10, 70, proposed, edge)]])
    assert o.shape == want.shape and (o == want).all()


# -------------------------------------------------------------------------------------------------------- run_slam

@pytest.fixture(scope="module")
def street():
    order = list(range(60)) + list(range(59, -1, -1))
    cache = {f: synth.lidar_frame(f, beams=32, azimuths=900, **synth.DRIVE_200) for f in set(order)}
    return [cache[f] for f in order]


@pytest.fixture(scope="module")
def plain_run(ctx, street):
    from lidar_slam_from_scratch_amd import slam
    return slam.run_slam(street, ctx)


def _same_factors(a, b):
    def same(x, y):
        return len(x) == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y))
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


def test_run_slam_without_a_gate_is_the_parents_run(ctx, street, plain_run):
    from lidar_slam_from_scratch_amd import slam
    run = slam.run_slam(street, ctx, closure_gate=None)
    assert run.closures and _same_factors(run.factors, plain_run.factors)
    assert [o[:2] for o in run.optimizations] == [o[:2] for o in plain_run.optimizations]
    assert [o[2].history for o in run.optimizations] == [o[2].history for o in plain_run.optimizations]
    assert (np.stack(run.poses) == np.stack(plain_run.poses)).all()
    assert run.rejected_closures == []


def test_run_slam_gate_keeps_a_false_closure_out(ctx, street, plain_run, monkeypatch):
    """One false closure injected into the first detect() that finds any: under a chi-squared gate it lands in
    rejected_closures, the true ones enter, and the final poses are those of the run that never saw it."""
    from lidar_slam_from_scratch_amd import loop_closure as lc
    from lidar_slam_from_scratch_amd import slam
    inner = lc.LoopClosureDetector.detect
    injected = []

    def detect(self):
        out = list(inner(self))
        if out and not injected:
            q = out[0].query_frame
            injected.append(lc.LoopClosureResult(q, q - 30, np.eye(4), 0.0, 0.0))   # 30 frames apart, "the same place"
            out.insert(1, injected[0])
        return out

    monkeypatch.setattr(lc.LoopClosureDetector, "detect", detect)
    run = slam.run_slam(street, ctx, closure_gate=M.CHI2_6_999)
    assert injected and [c for c, _ in run.rejected_closures] == injected
    print("rejected d2", [d for _, d in run.rejected_closures])
    assert all(d > M.CHI2_6_999 for _, d in run.rejected_closures)
    assert [(c.match_frame, c.query_frame) for c in run.closures] == \
        [(c.match_frame, c.query_frame) for c in plain_run.closures]
    assert _same_factors(run.factors, plain_run.factors)
    tags = [o[0] for o in run.optimizations]
    assert [t for t in tags if not isinstance(t, tuple)] == [o[0] for o in plain_run.optimizations]
    assert [t for t in tags if isinstance(t, tuple)] == [("gate", k) for k in sorted({c.query_frame for c in run.closures})]
    assert (np.stack(run.poses) == np.stack(plain_run.poses)).all()
