"""icpmi_last_normal_matrix on the device: the normal equations of the pass that produced final_error, through every
engine, both ways a loop ends and every entry point, against sums formed on the CPU.

Reference.  The source moved by the returned T in numpy, exact nearest neighbours from scipy's cKDTree (the parity tests
hold the engines to those indices), the oracle's normals (bit-equal to the device's, tests/test_gpu_parity.py), the
per-row terms w J_r J_c formed in numpy in the kernels' operation order, and math.fsum over the rows.

Tolerance per entry, derived, not tuned.
  (1) the device adds n rounded products in an order of its own: at most n 2^-52 sum |w J_r J_c| from the exact sum.
  (2) the device's rows are not T p: they were moved pass by pass by each step's update, and T is the rounded product of
      those updates.  One 3 x 4 transform of a point errs by at most 4 ulp of (sqrt(3) |p| + |t|) per coordinate (three
      products, three additions); over k passes for the rows, k products for T and once more for numpy's own T p:
          dp = 8 (k + 1) 2^-53 (sqrt(3) RHO + TAU)        per coordinate, RHO = max |T p|, TAU = max |t| over the passes
      J's rotation half is p x n with |n| = 1, so each of its entries moves by at most dJ = 2 sqrt(3) dp, its
      translation half (n itself) by nothing, and b = (q - p) . n by at most db = sqrt(3) dp.  An entry of JtJ then moves
      by at most sum w (|J_r| dJ_c + |J_c| dJ_r), of Jtb by sum w (|J_r| db + |b| dJ_r), sum b^2 by sum 2 w |b| db.
  (3) Huber's weight min(1, k / |b|) is Lipschitz in b with constant 1 / k: dw = db / k, which adds sum dw |J_r J_c|
      (likewise |J_r b| and b^2), and db / k per row to the weight sum.
The tolerance is (1) + (2) + (3); it comes to 1e-9 .. 1e-7 of entries of 1e5 .. 1e7."""
import math
import os
import sys

import numpy as np
import pytest

import torch  # noqa: F401  (first: one HIP runtime per process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402

pytestmark = pytest.mark.gpu

ENGINES = {"auto": capi.SEARCH_AUTO, "exact_f64": capi.SEARCH_EXACT_F64, "mfma_bf16": capi.SEARCH_MFMA_BF16,
           "mfma_pruned": capi.SEARCH_MFMA_PRUNED}
# (context, rows of source and target): the small-cloud kernel, all pairs, the culled engine; engines 1-3 by name
SHAPES = {"small_3000": ("auto", 3000), "all_pairs_20000": ("auto", 20000), "culled_30000": ("auto", 30000),
          "exact_20000": ("exact_f64", 20000), "mfma_20000": ("mfma_bf16", 20000), "pruned_20000": ("mfma_pruned", 20000)}
GATE, HUBER = 2.0, (capi.ROBUST_HUBER, 0.01)
U = 2.0 ** -53


@pytest.fixture(scope="module")
def contexts():
    """One context per search engine, made on first use (profile=1: the tests ask which kernels ran).  Fails loudly (no
    skip, no fallback) when the HIP library or the device is missing."""
    from lidar_slam_from_scratch_amd import build
    build.build_library()
    made = {}

    def get(engine):
        if engine not in made:
            made[engine] = capi.Context(device=0, search=ENGINES[engine], profile=1)
        return made[engine]

    yield get
    for c in made.values():
        c.close()


_pairs = {}


def pair(n, oracle):
    """The room-corner pair of n rows, its target's kd-tree and normals: computed once, shared, left unchanged."""
    if n not in _pairs:
        from scipy.spatial import cKDTree
        src, tgt, _ = synth.c1_room_corner(n)
        _pairs[n] = (src, tgt, cKDTree(tgt), oracle.estimate_normals(tgt, None, 20, nthreads=4))
    return _pairs[n]


def config(ending):
    """break: the default tolerance stops the loop; exhaust: three iterations with both tests off, then the post-loop pass"""
    if ending == "break":
        return capi.Context.make_config(max_iterations=50, tolerance=1e-6, min_error=1e-9)
    return capi.Context.make_config(max_iterations=3, tolerance=0.0, min_error=0.0)


def check(nm, res, src, tgt, tree, nrm, gate=None, huber=None):
    """The getter's record against the CPU sums; -> the largest error / tolerance over the 28 sums (printed by callers)."""
    T = np.array(res.transformation[:]).reshape(4, 4)
    assert np.array_equal(nm.T, T)
    assert np.array_equal(nm.JtJ, nm.JtJ.T)
    p = src @ T[:3, :3].T + T[:3, 3]
    d, j = tree.query(p)
    keep = np.ones(len(p), dtype=bool) if gate is None else d * d <= gate * gate
    p, q, n = p[keep], tgt[j[keep]], nrm[j[keep]]
    J = np.concatenate([np.cross(p, n), n], axis=1)
    dd = q - p
    b = (dd[:, 0] * n[:, 0] + dd[:, 1] * n[:, 1]) + dd[:, 2] * n[:, 2]
    w = np.ones(len(p))
    if huber is not None:
        a = np.abs(b)
        w = np.where(a <= huber, 1.0, huber / np.where(a <= huber, 1.0, a))
    rows = len(p)
    assert nm.pairs == rows
    passes = res.num_iterations + 1
    rho, tau = float(np.linalg.norm(p, axis=1).max()), 1.0          # (the pair's transform moves by 0.12 m: 1 m bounds it)
    dp = 8.0 * (passes + 1) * U * (math.sqrt(3.0) * rho + tau)
    dJ = np.r_[[2.0 * math.sqrt(3.0) * dp] * 3, [0.0] * 3]
    db = math.sqrt(3.0) * dp
    dw = db / huber if huber is not None else 0.0
    wJ = w[:, None] * J                                              # the kernels' order: (w J_r) J_c, (w J_r) b, (w b) b
    worst = 0.0

    def held(got, terms, moved):
        nonlocal worst
        want = math.fsum(terms)
        tol = rows * 2.0 * U * float(np.sum(np.abs(terms))) + moved
        worst = max(worst, abs(got - want) / tol)
        assert abs(got - want) <= tol, (got, want, abs(got - want), tol)

    aJ, ab = np.abs(J), np.abs(b)
    for r in range(6):
        for c in range(r, 6):
            held(nm.JtJ[r, c], wJ[:, r] * J[:, c],
                 float(np.sum(w * (aJ[:, r] * dJ[c] + aJ[:, c] * dJ[r]) + dw * aJ[:, r] * aJ[:, c])))
        held(nm.Jtb[r], wJ[:, r] * b, float(np.sum(w * (aJ[:, r] * db + ab * dJ[r]) + dw * aJ[:, r] * ab)))
    held(nm.sum_sq, (w * b) * b, float(np.sum(2.0 * w * ab * db + dw * ab * ab)))
    if huber is None:
        assert nm.weight == float(rows)
    else:
        held(nm.weight, w, rows * dw)
    assert math.sqrt(nm.sum_sq / nm.weight) == res.final_error       # to the bit, through the sqrt
    return worst


def _bits(nm):
    return (nm.JtJ.tobytes(), nm.Jtb.tobytes(), nm.sum_sq, nm.weight, nm.pairs, nm.T.tobytes())


@pytest.mark.parametrize("ending", ["break", "exhaust"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_plain_call(contexts, oracle, shape, ending):
    engine, n = SHAPES[shape]
    c = contexts(engine)
    src, tgt, tree, nrm = pair(n, oracle)
    cfg = config(ending)
    c.reset_profile()
    res, hist = c.align(src, tgt, cfg)
    prof = c.get_profile()
    assert (prof["small_launches"] > 0) == (shape == "small_3000")
    assert (prof["nn_group_pairs"] > 0) == (shape in ("culled_30000", "pruned_20000"))
    if ending == "break":
        assert res.converged and res.loop_iterations < cfg.max_iterations
    else:
        assert not res.converged and res.loop_iterations == 3 and res.num_iterations == 3
    worst = check(c.last_normal_matrix(), res, src, tgt, tree, nrm)
    print(shape, ending, "iterations", res.num_iterations, "rms", res.final_error, "worst error / tolerance", worst)
    assert _bits(c.last_normal_matrix()) == _bits(c.last_normal_matrix(0))      # reading it changes nothing


@pytest.mark.parametrize("ending", ["break", "exhaust"])
@pytest.mark.parametrize("shape", ["small_3000", "all_pairs_20000"])
def test_gated_and_huber_calls(contexts, oracle, shape, ending):
    engine, n = SHAPES[shape]
    c = contexts(engine)
    src, tgt, tree, nrm = pair(n, oracle)
    cfg = config(ending)
    res, _hist, pairs = c.align_gated(src, tgt, cfg, GATE)
    nm = c.last_normal_matrix()
    assert nm.pairs == pairs
    worst_g = check(nm, res, src, tgt, tree, nrm, gate=GATE)
    res, _hist, info = c.align_robust(src, tgt, cfg, HUBER)
    nm = c.last_normal_matrix()
    assert nm.pairs == info.pairs and nm.weight == info.weight_sum and nm.weight < nm.pairs     # some rows are down-weighted
    worst_h = check(nm, res, src, tgt, tree, nrm, huber=HUBER[1])
    print(shape, ending, "worst error / tolerance: gated", worst_g, "huber", worst_h)


def test_batch_of_three_is_each_call_alone(contexts, oracle):
    c = contexts("auto")
    sizes = [3000, 20000, 3000]
    srcs = [pair(n, oracle)[0] for n in sizes]
    tgts = [pair(n, oracle)[1] for n in sizes]
    srcs[2] = srcs[2] + np.array([0.05, 0.0, 0.02])                 # a third problem of its own
    cfgs = [config("break"), config("exhaust"), config("break")]
    alone = []
    for s, t, cfg in zip(srcs, tgts, cfgs):
        c.align(s, t, cfg)
        alone.append(_bits(c.last_normal_matrix()))
    out = c.align_batch(srcs, tgts, cfgs)
    for k in range(3):
        nm = c.last_normal_matrix(k)
        assert _bits(nm) == alone[k]
        assert np.array_equal(nm.T, np.array(out[k][0].transformation[:]).reshape(4, 4))
    with pytest.raises(capi.IcpError) as e:
        c.last_normal_matrix(3)
    assert e.value.code == capi.ERR_ARG
    worst = check(c.last_normal_matrix(1), out[1][0], srcs[1], tgts[1], pair(20000, oracle)[2], pair(20000, oracle)[3])
    print("batch: worst error / tolerance", worst)
    c.align(srcs[0], tgts[0], cfgs[0])                               # a single call again: problem 0 only
    assert _bits(c.last_normal_matrix()) == alone[0]
    with pytest.raises(capi.IcpError):
        c.last_normal_matrix(1)


@pytest.mark.parametrize("shape", ["small_3000", "culled_30000"])
def test_device_pointer_entry(contexts, oracle, shape):
    engine, n = SHAPES[shape]
    c = contexts(engine)
    src, tgt, tree, nrm = pair(n, oracle)
    cfg = config("break")
    c.align(src, tgt, cfg)
    host = _bits(c.last_normal_matrix())
    ds, dt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    torch.cuda.synchronize()
    res, _hist = c.align_device(ds.data_ptr(), n, dt.data_ptr(), n, cfg)
    nm = c.last_normal_matrix()
    assert _bits(nm) == host
    check(nm, res, src, tgt, tree, nrm)


def test_stream_push(contexts, oracle):
    from scipy.spatial import cKDTree
    c = contexts("auto")
    cfg = capi.Context.make_config()
    frames = [synth.lidar_frame(f, beams=32, azimuths=900, **synth.DRIVE_200) for f in (0, 1)]
    c.stream_reset()
    c.align(*pair(3000, oracle)[:2], config("break"))               # a registration before the stream starts ...
    _res, _hist, info = c.stream_push_host(frames[0], 0.5, 1000, cfg)
    assert info.status == capi.STREAM_FIRST_FRAME
    with pytest.raises(capi.IcpError) as e:                          # ... is not what a push that registered nothing left
        c.last_normal_matrix()
    assert e.value.code == capi.ERR_ARG
    target = c.stream_current_scan()
    res, _hist, info = c.stream_push_host(frames[1], 0.5, 1000, cfg)
    assert info.status == capi.STREAM_REGISTERED
    source = c.stream_current_scan()
    nm = c.last_normal_matrix()
    worst = check(nm, res, source, target, cKDTree(target), oracle.estimate_normals(target, None, 20, nthreads=4))
    print("stream: rows", len(source), "->", len(target), "worst error / tolerance", worst)
    _res, _hist, info = c.stream_push_host(frames[1][:500], 0.5, 1000, cfg)
    assert info.status == capi.STREAM_TOO_FEW_POINTS
    with pytest.raises(capi.IcpError):
        c.last_normal_matrix()
    c.stream_reset()


def test_errors(contexts):
    from lidar_slam_from_scratch_amd import build
    build.build_library()
    fresh = capi.Context(device=0)
    try:
        with pytest.raises(capi.IcpError) as e:                      # no registration ran
            fresh.last_normal_matrix()
        assert e.value.code == capi.ERR_ARG and "normal matrix" in str(e.value)
        rng = np.random.default_rng(3)
        a = rng.uniform(0, 10, (1500, 3))
        res, _hist, pairs = fresh.align_gated(a + 100.0, a, capi.Context.make_config(), 0.5)   # a gate that keeps no row
        assert pairs == 0 and math.isinf(res.final_error)
        with pytest.raises(capi.IcpError) as e:
            fresh.last_normal_matrix()
        assert e.value.code == capi.ERR_ARG
        with pytest.raises(capi.IcpError):
            fresh.last_normal_matrix(-1)
    finally:
        fresh.close()
