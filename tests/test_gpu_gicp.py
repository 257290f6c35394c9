"""Plane-to-plane ICP on the device: k_reduce_gicp behind icpmi_align_gicp / _device, with the source's
normals estimated on the device in front of the target's preparation.  On scripts/gicp_ref.py's fixtures the library agrees
with the CPU restatement within tests/test_gpu_parity.py's tolerances on the three engines and on AUTO, takes the same
passes and keeps the same rows, and the engines agree with each other bit for bit; a start that is not the identity;
epsilon = 1 through icpmi_last_normal_matrix; a pass without pairs; device pointers; a used context; odometry and the
SLAM driver; the error codes."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import torch  # noqa: F401  (first: one HIP runtime per process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import gicp_ref as ref  # noqa: E402
import robust_icp_ref as rr  # noqa: E402
from lidar_slam_from_scratch_amd import capi, odometry, slam, synth  # noqa: E402

pytestmark = pytest.mark.gpu

POSE_TOL_M, POSE_TOL_RAD, HIST_ATOL = 1e-4, 1e-4, 1e-9   # tests/test_gpu_parity.py's
ENGINES = {"auto": capi.SEARCH_AUTO, "exact_f64": capi.SEARCH_EXACT_F64, "mfma_bf16": capi.SEARCH_MFMA_BF16,
           "mfma_pruned": capi.SEARCH_MFMA_PRUNED}
FIXTURES = ["sub_1001_1500", "sub_1001_1500_start", "sub_33_700", "sub_5_700", "c2", "cars", "uniform_65537_20000"]
DRIVE_FRAMES = 12
ODOM_RULE = (1e-3, 2.0)


@pytest.fixture(scope="module")
def contexts():
    """One context per search engine, made on first use.  Fails loudly (no skip, no fallback) when the HIP library or
    the device is missing.  profile=1: the tests ask which kernels ran."""
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


@pytest.fixture(scope="module")
def ctx(contexts):
    return contexts("auto")


@pytest.fixture(scope="module")
def fixtures():
    return ref.gpu_fixtures()


@pytest.fixture(scope="module")
def wants(oracle, fixtures):
    """name -> the restatement's result, once"""
    return {name: ref.run_fixture(f, oracle) for name, f in fixtures.items()}


@pytest.fixture(scope="module")
def runs(contexts, fixtures):
    """(fixture, engine) -> the library's outcome, each computed once: the parity test and the engines' comparison share
    them.  The call's own profile is taken with it: get.small[(fixture, engine)] is its small-cloud launches."""
    done, small = {}, {}

    def get(name, engine):
        if (name, engine) not in done:
            c = contexts(engine)
            c.reset_profile()
            done[(name, engine)] = _call(c, fixtures[name])
            small[(name, engine)] = c.get_profile()["small_launches"]
        return done[(name, engine)]

    get.small = small

    return get


def _cfg(f):
    return capi.Context.make_config(f["max_iterations"], 1e-6, 1e-9, f["start"])


def _rule(f):
    return (f["epsilon"], f["gate"])


def _call(c, f):
    return c.align_gicp(f["source"], f["target"], _cfg(f), _rule(f))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _T(res):
    return np.array(res.transformation[:]).reshape(4, 4)


def _same_bits(a, b):
    """two (Result, history, GicpInfo) outcomes"""
    assert np.array_equal(_bits(_T(a[0])), _bits(_T(b[0])))
    assert np.array_equal(_bits(a[1]), _bits(b[1]))
    assert (a[0].converged, a[0].num_iterations, a[0].history_len, a[0].loop_iterations) == \
        (b[0].converged, b[0].num_iterations, b[0].history_len, b[0].loop_iterations)
    assert _bits([a[0].final_error]) == _bits([b[0].final_error])
    assert (a[2].pairs, a[2].rows) == (b[2].pairs, b[2].rows)


# ------------------------------------------------------------------------------------------------ the restatement

@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", FIXTURES)
def test_parity_with_the_restatement(contexts, fixtures, wants, runs, name, engine):
    f, want = fixtures[name], wants[name]
    res, hist, info = runs(name, engine)
    assert runs.small[(name, engine)] == 0               # no small-cloud form, at any size (that call's own profile)
    dt, dr = synth.pose_delta(_T(res), want.transformation)
    print("  %s on %s: %.3e m %.3e rad, history differs by %.3e, pairs %d / %d, iterations %d / %d"
          % (name, engine, dt, dr, np.abs(hist - want.error_history).max() if len(hist) == len(want.error_history) else math.nan,
             info.pairs, want.pairs, res.num_iterations, want.num_iterations))
    assert res.num_iterations == want.num_iterations and bool(res.converged) == want.converged
    assert info.pairs == want.pairs and info.rows == f["source"].shape[0]
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD
    assert np.allclose(hist, want.error_history, rtol=0.0, atol=HIST_ATOL)
    assert abs(res.final_error - want.final_error) <= HIST_ATOL


@pytest.mark.parametrize("name", FIXTURES)
def test_engines_agree_bit_for_bit(runs, name):
    """the matches are exact on every engine, the normals bit-exact, and k_reduce_gicp's grid does not depend on the engine"""
    first = runs(name, "exact_f64")
    for engine in ("mfma_bf16", "mfma_pruned", "auto"):
        _same_bits(runs(name, engine), first)


def test_the_start_takes_part(fixtures, runs):
    """sub_1001_1500_start is sub_1001_1500 with the source moved by the inverse of its start, 1.3 rad away: the same
    problem up to the rounding of that move, so the same passes and rows and the pose composed with the start -- but only
    if the source's normals, estimated on the rows as the caller gave them, are turned by R"""
    a, b = runs("sub_1001_1500", "exact_f64"), runs("sub_1001_1500_start", "exact_f64")
    start = np.asarray(fixtures["sub_1001_1500_start"]["start"])
    assert math.acos((np.trace(start[:3, :3]) - 1.0) / 2.0) > 1.0
    dt, dr = synth.pose_delta(_T(a[0]) @ start, _T(b[0]))
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD
    assert a[2].pairs == b[2].pairs and a[0].num_iterations == b[0].num_iterations
    assert np.allclose(a[1], b[1], rtol=0.0, atol=HIST_ATOL)


# ------------------------------------------------------------------------------------------------ edges

@pytest.mark.parametrize("engine", ["auto", "exact_f64"])
def test_epsilon_one_is_point_to_point_exactly(contexts, fixtures, engine):
    c = contexts(engine)
    f = dict(fixtures["sub_1001_1500"], epsilon=1.0)
    res, _hist, info = _call(c, f)
    nm = c.last_normal_matrix()
    assert info.pairs > 0 and nm.pairs == info.pairs and nm.weight == float(info.pairs)
    assert nm.JtJ[3, 3] == nm.JtJ[4, 4] == nm.JtJ[5, 5] == info.pairs / 2.0
    assert nm.JtJ[3, 4] == 0.0 and nm.JtJ[3, 5] == 0.0 and nm.JtJ[4, 5] == 0.0
    assert res.final_error == math.sqrt(nm.sum_sq / nm.weight) and np.array_equal(nm.T, _T(res))


def test_last_normal_matrix_is_the_last_passes(ctx, fixtures, wants):
    f, want = fixtures["cars"], wants["cars"]
    res, _hist, info = _call(ctx, f)
    nm = ctx.last_normal_matrix()
    assert nm.pairs == info.pairs == want.pairs and nm.weight == float(want.pairs)
    assert res.final_error == math.sqrt(nm.sum_sq / nm.weight)
    assert np.array_equal(nm.JtJ, nm.JtJ.T) and np.array_equal(nm.T, _T(res))
    assert (np.linalg.eigvalsh(nm.JtJ) > 0.0).all()


@pytest.mark.parametrize("engine", ["auto", "exact_f64"])
def test_no_pairs_ends_the_call(contexts, fixtures, wants, engine):
    c = contexts(engine)
    f = fixtures["sub_1001_1500"]
    far = f["source"] + np.array([500.0, 0.0, 0.0])
    res, hist, info = c.align_gicp(far, f["target"], capi.Context.make_config(), (1e-3, 1.0))
    assert hist.tolist() == [math.inf, math.inf] and res.final_error == math.inf
    assert not res.converged and res.num_iterations == 1 and res.loop_iterations == 1
    assert info.pairs == 0 and info.rows == far.shape[0] and np.array_equal(_T(res), np.eye(4))
    with pytest.raises(capi.IcpError) as e:
        c.last_normal_matrix()
    assert e.value.code == capi.ERR_ARG
    res, hist, info = c.align_gicp(far, f["target"], capi.Context.make_config(max_iterations=0), (1e-3, 1.0))
    assert hist.tolist() == [math.inf] and res.num_iterations == 0 and not res.converged and info.pairs == 0
    res, _hist, info = _call(c, f)                       # and the context goes on as before
    assert res.converged and info.pairs == wants["sub_1001_1500"].pairs


def test_device_pointers_give_the_host_call(ctx, fixtures):
    f = fixtures["cars"]
    ds, dt_ = torch.from_numpy(f["source"]).cuda(), torch.from_numpy(f["target"]).cuda()
    torch.cuda.synchronize()
    got = ctx.align_gicp_device(ds.data_ptr(), f["source"].shape[0], dt_.data_ptr(), f["target"].shape[0], _cfg(f), _rule(f))
    _same_bits(got, _call(ctx, f))
    assert np.array_equal(ds.cpu().numpy(), f["source"]) and np.array_equal(dt_.cpu().numpy(), f["target"])


@pytest.mark.parametrize("engine", ["auto", "mfma_bf16"])
def test_a_used_context_gives_a_fresh_ones_bits(fixtures, engine):
    """a plain align, then align_gicp, then the plain align against the same target again: src_nrm, the source's search
    structure and the forgotten target leak nothing in either direction"""
    f, other = fixtures["c2"], fixtures["sub_1001_1500"]
    cfg = capi.Context.make_config()

    def fresh(call):
        c = capi.Context(device=0, search=ENGINES[engine])
        try:
            return call(c)
        finally:
            c.close()

    def plain(c):
        return c.align(f["source"], f["target"], cfg)

    want_plain, want_gicp, want_other = fresh(plain), fresh(lambda c: _call(c, f)), fresh(lambda c: _call(c, other))
    used = capi.Context(device=0, search=ENGINES[engine])
    try:
        a = plain(used)
        b = _call(used, f)
        c2 = plain(used)
        d = _call(used, other)                           # a smaller pair behind a larger one: stale rows of src_nrm
        e = _call(used, f)
    finally:
        used.close()
    for got in (a, c2):
        assert np.array_equal(_bits(_T(got[0])), _bits(_T(want_plain[0]))) and np.array_equal(_bits(got[1]), _bits(want_plain[1]))
        assert got[0].num_iterations == want_plain[0].num_iterations
    _same_bits(b, want_gicp)
    _same_bits(e, want_gicp)
    _same_bits(d, want_other)


# ------------------------------------------------------------------------------------------------ odometry

def test_odometry_reproduces_the_restatement(ctx, oracle):
    frames, poses = rr.drive_frames(DRIVE_FRAMES)
    want = rr.odometry_ate(frames, poses, ref.gicp_align(*ODOM_RULE, orc=oracle))
    align = odometry.gpu_align(ctx, gicp=ODOM_RULE)
    track = odometry.run_odometry(frames, align)
    got = odometry.absolute_trajectory_error(track, poses)
    print("  drive 0..%d plane-to-plane behind %.0f m: ATE rms %.6f m on the device, %.6f m restated, %d / %d passes"
          % (DRIVE_FRAMES - 1, ODOM_RULE[1], got, want[0], sum(track.iterations), want[2]))
    assert abs(got - want[0]) <= 1e-6 and sum(track.iterations) == want[2] and not any(track.gated)
    r = align(frames[1], frames[0], 50, 1e-6)
    assert 0 < r.pairs <= frames[1].shape[0]
    run = slam.run_slam(frames, ctx, odom_gicp=ODOM_RULE)
    # the node's loop registers the same pairs: its odometry factors are the track's deltas bit for bit, and its poses --
    # what the pose graph returns for a chain without closures, whose optimum is the chain itself -- the track's within
    # the tolerance above
    odom = [f for f in run.factors if f[0] == "odom"]
    assert len(run.poses) == len(track.poses) and len(odom) == len(track.deltas) and not run.closures
    assert all(np.array_equal(_bits(f[3]), _bits(d)) for f, d in zip(odom, track.deltas))
    assert max(np.linalg.norm(np.asarray(x)[:3, 3] - y[:3, 3]) for x, y in zip(run.poses, track.poses)) <= 1e-6
    with pytest.raises(ValueError):
        odometry.gpu_align(ctx, gicp=ODOM_RULE, robust=(capi.ROBUST_HUBER, 0.1))
    with pytest.raises(ValueError):
        slam.run_slam(frames[:2], ctx, odom_gicp=ODOM_RULE, odom_robust=(capi.ROBUST_HUBER, 0.1))
    with pytest.raises(ValueError):
        slam.run_slam(frames[:2], ctx, odom_gicp=ODOM_RULE, align=align)


# ------------------------------------------------------------------------------------------------ error codes

def test_error_codes(ctx, fixtures):
    lib = capi.load_library()
    f = fixtures["sub_33_700"]
    src, tgt = f["source"], f["target"]
    cfg = capi.Context.make_config()
    for bad in ((0.0,), (-1e-3,), (1.0 + 1e-12,), (math.nan,), (math.inf,), (-math.inf,), (1e-3, -2.0), (1e-3, math.nan),
                (1e-3, math.inf)):
        with pytest.raises(capi.IcpError) as e:
            ctx.align_gicp(src, tgt, cfg, bad)
        assert e.value.code == capi.ERR_ARG, bad
    hist, res = np.zeros(51), capi.Result()
    assert lib.icpmi_align_gicp(ctx._h, capi._dp(src), 33, capi._dp(tgt), 700, C.byref(cfg), None, C.byref(res), None,
                                capi._dp(hist), 51) == capi.ERR_NULL       # no rule: that is icpmi_align
    rule = capi.as_gicp((1.0,))                                            # epsilon = 1 is allowed
    assert lib.icpmi_align_gicp(ctx._h, capi._dp(src), 33, capi._dp(tgt), 700, C.byref(cfg), C.byref(rule), C.byref(res),
                                None, capi._dp(hist), 51) == capi.OK       # info may be NULL
    assert lib.icpmi_align_gicp(ctx._h, capi._dp(src), 33, capi._dp(tgt), 700, C.byref(cfg), C.byref(rule), C.byref(res),
                                None, capi._dp(hist), 50) == capi.ERR_CAPACITY
    assert lib.icpmi_align_gicp(None, capi._dp(src), 33, capi._dp(tgt), 700, C.byref(cfg), C.byref(rule), C.byref(res),
                                None, capi._dp(hist), 51) == capi.ERR_NULL
    # a context with a communicator (the callbacks form, one rank) does not run plane-to-plane registrations
    c = capi.Context(device=0)
    c.comm_init_callbacks(1, 0, lambda buf: None, lambda buf, per: None)
    with pytest.raises(capi.IcpError) as e:
        c.align_gicp(src, tgt, cfg, (1e-3,))
    assert e.value.code == capi.ERR_ARG
    c.comm_finalize()
    res, _hist, info = c.align_gicp(src, tgt, cfg, (1e-3,))            # and does again without one
    assert res.converged and info.pairs == 33
    c.close()
