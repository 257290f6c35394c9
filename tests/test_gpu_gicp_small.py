"""Plane-to-plane ICP in the small-cloud kernel: k_icp_small_gicp behind ICPMI_GICP_FORM_SMALL, through
icpmi_align_gicp / _device / _batch and icpmi_loop_set_gicp.  With the flag the kernel runs at the small-cloud kernel's
sizes and nowhere else; without it a call is what it was.  On scripts/gicp_ref.py's small fixtures and at the block edges
the flagged calls agree with the CPU restatement within tests/test_gpu_gicp.py's bounds, take the same passes and keep
the same rows; epsilon = 1 exactly; a row of NaNs, a pass without pairs; device pointers, a used context, the batch;
both loop detectors on L12, the C++ mirror, set_gicp(0), the information matrices; run_slam; the error codes."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import torch  # noqa: F401  (first: one HIP runtime per process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import gated_icp_ref as gr  # noqa: E402
import gicp_ref as ref  # noqa: E402
import loop_yaw_ref as yr  # noqa: E402
import robust_icp_ref as rr  # noqa: E402
from lidar_slam_from_scratch_amd import capi, slam, synth  # noqa: E402
from lidar_slam_from_scratch_amd import loop_closure as lc  # noqa: E402
from lidar_slam_from_scratch_amd.global_map import GlobalMap  # noqa: E402

pytestmark = pytest.mark.gpu

POSE_TOL_M, POSE_TOL_RAD, HIST_ATOL = 1e-4, 1e-4, 1e-9   # tests/test_gpu_gicp.py's, which are tests/test_gpu_parity.py's
ENGINES = {"auto": capi.SEARCH_AUTO, "mfma_bf16": capi.SEARCH_MFMA_BF16}
SMALL_FIXTURES = ["sub_1001_1500", "sub_1001_1500_start", "sub_33_700", "sub_5_700", "c2", "cars"]
EDGE_ROWS = [1, 31, 32, 33, 1001]
GATE = gr.L12_GATE
EPS = ref.EPSILON_DEFAULT
MFMA_MIN_ROWS = 64   # AUTO takes the exact fp64 engine, which has no small-cloud kernel, for sources of fewer rows


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
    """gicp_ref.gpu_fixtures() plus the block edges (n rows of the C2 pair against 1,500 targets behind the fixtures' gate)
    and the two pairs the small-cloud kernel does not reach"""
    out = ref.gpu_fixtures()
    for n in EDGE_ROWS[:-1]:
        s, t, _ = ref.subsample_pair(n, 1500)
        out["edge_%d" % n] = dict(source=s, target=t, start=None, epsilon=EPS, gate=ref.FIXTURE_GATE, max_iterations=50)
    out["edge_1001"] = out["sub_1001_1500"]
    s, t, _ = ref.subsample_pair(1001, 4500)
    out["sub_1001_4500"] = dict(source=s, target=t, start=None, epsilon=EPS, gate=ref.FIXTURE_GATE, max_iterations=50)
    s, t, _ = synth.c3_uniform(16385, seed=71, perm_seed=72)
    out["uniform_5000_16385"] = dict(source=np.ascontiguousarray(s[:5000]), target=t, start=None, epsilon=EPS, gate=0.0,
                                     max_iterations=3)
    return out


@pytest.fixture(scope="module")
def wants(oracle, fixtures):
    """name -> the restatement's result, each computed on first use"""
    done = {}

    def get(name):
        if name not in done:
            done[name] = ref.run_fixture(fixtures[name], oracle)
        return done[name]

    return get


@pytest.fixture(scope="module")
def l12():
    return gr.l12_scans()


def _cfg(f):
    return capi.Context.make_config(f["max_iterations"], 1e-6, 1e-9, f["start"])


def _rule(f, small=True):
    return (f["epsilon"], f["gate"], small)


def _call(c, f, small=True):
    return c.align_gicp(f["source"], f["target"], _cfg(f), _rule(f, small))


def _ran(c, call):
    """-> (call(), the small-cloud launches it made)"""
    c.reset_profile()
    out = call()
    return out, c.get_profile()["small_launches"]


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


def _against_restatement(name, engine, got, want, rows):
    res, hist, info = got
    dt, dr = synth.pose_delta(_T(res), want.transformation)
    print("  %s on %s: %.3e m %.3e rad, history differs by %.3e, pairs %d / %d, iterations %d / %d"
          % (name, engine, dt, dr, np.abs(hist - want.error_history).max() if len(hist) == len(want.error_history) else math.nan,
             info.pairs, want.pairs, res.num_iterations, want.num_iterations))
    assert res.num_iterations == want.num_iterations and bool(res.converged) == want.converged
    assert info.pairs == want.pairs and info.rows == rows
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD
    assert np.allclose(hist, want.error_history, rtol=0.0, atol=HIST_ATOL)
    assert abs(res.final_error - want.final_error) <= HIST_ATOL


# ------------------------------------------------------------------------------------------------ the kernel runs

@pytest.mark.parametrize("name", ["sub_1001_1500", "sub_1001_4500"])
def test_the_flag_selects_the_kernel(ctx, fixtures, name):
    """one split, and three with the last ragged (4,500 = 2 x 2,048 + 404).  Fails on a library without the small form."""
    f = fixtures[name]
    flagged, small = _ran(ctx, lambda: _call(ctx, f))
    assert small > 0
    plain, small = _ran(ctx, lambda: _call(ctx, f, small=False))
    assert small == 0
    # the other bits of `reserved` are ignored, and a two-element rule is the unflagged one
    rule = capi.as_gicp((f["epsilon"], f["gate"]))
    rule.reserved = ~capi.GICP_FORM_SMALL
    other, small = _ran(ctx, lambda: ctx.align_gicp(f["source"], f["target"], _cfg(f), rule))
    assert small == 0
    _same_bits(other, plain)
    _same_bits(ctx.align_gicp(f["source"], f["target"], _cfg(f), (f["epsilon"], f["gate"])), plain)
    # the two forms: the same passes and rows, to rounding the same pose
    assert flagged[0].num_iterations == plain[0].num_iterations and flagged[2].pairs == plain[2].pairs
    dt, dr = synth.pose_delta(_T(flagged[0]), _T(plain[0]))
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD and np.allclose(flagged[1], plain[1], rtol=0.0, atol=HIST_ATOL)


# ------------------------------------------------------------------------------------------------ the restatement

@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", SMALL_FIXTURES)
def test_parity_with_the_restatement(contexts, fixtures, wants, name, engine):
    c, f = contexts(engine), fixtures[name]
    got, small = _ran(c, lambda: _call(c, f))
    assert (small > 0) == (engine == "mfma_bf16" or f["source"].shape[0] >= MFMA_MIN_ROWS)
    _against_restatement(name, engine, got, wants(name), f["source"].shape[0])


@pytest.mark.parametrize("n", EDGE_ROWS)
def test_block_edges(contexts, fixtures, wants, n):
    """a workgroup of one valid row, one short of full, full, and one row into the second"""
    c, f = contexts("mfma_bf16"), fixtures["edge_%d" % n]
    got, small = _ran(c, lambda: _call(c, f))
    assert small > 0
    _against_restatement("edge_%d" % n, "mfma_bf16", got, wants("edge_%d" % n), n)


@pytest.mark.parametrize("name", ["uniform_65537_20000", "uniform_5000_16385"])
def test_the_flag_has_no_effect_past_the_small_kernel(ctx, fixtures, name):
    """more than 32,768 rows; nine splits"""
    f = fixtures[name]
    flagged, small = _ran(ctx, lambda: _call(ctx, f))
    assert small == 0
    _same_bits(flagged, _call(ctx, f, small=False))


# ------------------------------------------------------------------------------------------------ edges

def test_epsilon_one_is_point_to_point_exactly(ctx, fixtures):
    f = dict(fixtures["sub_1001_1500"], epsilon=1.0)
    (res, _hist, info), small = _ran(ctx, lambda: _call(ctx, f))
    nm = ctx.last_normal_matrix()
    assert small > 0 and info.pairs > 0 and nm.pairs == info.pairs and nm.weight == float(info.pairs)
    assert nm.JtJ[3, 3] == nm.JtJ[4, 4] == nm.JtJ[5, 5] == info.pairs / 2.0
    assert nm.JtJ[3, 4] == 0.0 and nm.JtJ[3, 5] == 0.0 and nm.JtJ[4, 5] == 0.0
    assert res.final_error == math.sqrt(nm.sum_sq / nm.weight) and np.array_equal(nm.T, _T(res))
    assert np.array_equal(nm.JtJ, nm.JtJ.T)


def test_a_row_of_nans_is_dropped(ctx, fixtures):
    f = fixtures["sub_1001_1500"]
    n = f["source"].shape[0]
    bad = dict(f, source=np.insert(f["source"], n // 2, np.nan, axis=0), gate=0.0)
    (res, hist, info), small = _ran(ctx, lambda: _call(ctx, bad))
    want = _call(ctx, dict(f, gate=0.0))
    assert small > 0 and info.pairs == n and info.rows == n + 1 and want[2].pairs == n   # n - 1 of the n rows handed in
    dt, dr = synth.pose_delta(_T(res), _T(want[0]))
    assert res.num_iterations == want[0].num_iterations and res.converged == want[0].converged == 1
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD and np.allclose(hist, want[1], rtol=0.0, atol=HIST_ATOL)


def test_no_pairs_ends_the_call(ctx, fixtures, wants):
    f = fixtures["sub_1001_1500"]
    far = f["source"] + np.array([500.0, 0.0, 0.0])
    (res, hist, info), small = _ran(ctx, lambda: ctx.align_gicp(far, f["target"], capi.Context.make_config(), (EPS, 1.0, True)))
    assert small > 0
    assert hist.tolist() == [math.inf, math.inf] and res.final_error == math.inf
    assert not res.converged and res.num_iterations == 1 and res.loop_iterations == 1
    assert info.pairs == 0 and info.rows == far.shape[0] and np.array_equal(_T(res), np.eye(4))
    with pytest.raises(capi.IcpError) as e:
        ctx.last_normal_matrix()
    assert e.value.code == capi.ERR_ARG
    res, hist, info = ctx.align_gicp(far, f["target"], capi.Context.make_config(max_iterations=0), (EPS, 1.0, True))
    assert hist.tolist() == [math.inf] and res.num_iterations == 0 and not res.converged and info.pairs == 0
    res, _hist, info = _call(ctx, f)                     # and the context goes on as before
    assert res.converged and info.pairs == wants("sub_1001_1500").pairs


# ------------------------------------------------------------------------------------------------ bits across calls and forms

def test_device_pointers_give_the_host_call(ctx, fixtures):
    f = fixtures["cars"]
    ds, dt_ = torch.from_numpy(f["source"]).cuda(), torch.from_numpy(f["target"]).cuda()
    torch.cuda.synchronize()
    got, small = _ran(ctx, lambda: ctx.align_gicp_device(ds.data_ptr(), f["source"].shape[0], dt_.data_ptr(), f["target"].shape[0],
                                                         _cfg(f), _rule(f)))
    assert small > 0
    _same_bits(got, _call(ctx, f))
    assert np.array_equal(ds.cpu().numpy(), f["source"]) and np.array_equal(dt_.cpu().numpy(), f["target"])


@pytest.mark.parametrize("engine", list(ENGINES))
def test_a_used_context_gives_a_fresh_ones_bits(fixtures, engine):
    """a plain align, a general plane-to-plane call, the small form, a gated small call and the small form again: src_nrm,
    the source's search structure, the sorted normals and the partial rows leak nothing between the forms"""
    f, other = fixtures["sub_1001_4500"], fixtures["sub_1001_1500"]
    cfg = capi.Context.make_config()

    def fresh(call):
        c = capi.Context(device=0, search=ENGINES[engine])
        try:
            return call(c)
        finally:
            c.close()

    want_small, want_other = fresh(lambda c: _call(c, f)), fresh(lambda c: _call(c, other))
    want_general = fresh(lambda c: _call(c, f, small=False))
    used = capi.Context(device=0, search=ENGINES[engine])
    try:
        used.align(f["source"], f["target"], cfg)
        a = _call(used, f, small=False)
        b = _call(used, f)
        used.align_gated(f["source"], f["target"], cfg, GATE)
        c2 = _call(used, f)
        d = _call(used, other)                           # a smaller target behind a larger one
        e = _call(used, f)
    finally:
        used.close()
    _same_bits(a, want_general)
    for got in (b, c2, e):
        _same_bits(got, want_small)
    _same_bits(d, want_other)


def test_batch_is_the_calls_alone_bit_for_bit(ctx, fixtures):
    """flagged, unflagged, another epsilon"""
    f, g = fixtures["sub_1001_4500"], fixtures["sub_1001_1500_start"]
    probs = [(f, _rule(f)), (f, _rule(f, small=False)), (g, (0.25, g["gate"], True))]
    together = ctx.align_gicp_batch([p["source"] for p, _ in probs], [p["target"] for p, _ in probs],
                                    [_cfg(p) for p, _ in probs], [r for _, r in probs])
    for (p, rule), got in zip(probs, together):
        _same_bits(got, ctx.align_gicp(p["source"], p["target"], _cfg(p), rule))
    assert together[0][2].pairs > 0 and together[2][0].converged


# ------------------------------------------------------------------------------------------------ the detectors

def _key(r):
    return (r.query_frame, r.match_frame, r.sector_shift, r.pairs)


def _same_results(a, b):
    assert [_key(r) for r in a] == [_key(r) for r in b]
    for x, y in zip(a, b):
        assert x.weight_sum is None and y.weight_sum is None
        assert _bits([x.scan_context_distance]) == _bits([y.scan_context_distance])
        assert _bits([x.icp_fitness]) == _bits([y.icp_fitness])
        assert np.array_equal(_bits(x.transform), _bits(y.transform))
        assert (x.information is None) == (y.information is None)
        assert x.information is None or np.array_equal(_bits(x.information), _bits(y.information))


def _host_and_store(ctx, clouds, labels, cfg):
    """tests/test_gpu_loop_store.py's idiom: both detectors fed the same frames, a store frame of one row first"""
    store = GlobalMap(ctx)
    store.add_frame(np.array([[3.0, 4.0, 1.5]]))
    host, dev = lc.LoopClosureDetector(lc.GpuBackend(ctx), cfg), lc.StoreLoopClosureDetector(ctx, store, cfg)
    found = []
    for cloud, label in zip(clouds, labels):
        store.add_frame(cloud)
        host.add_frame(cloud, label)
        dev.add_frame(store.size()[0] - 1, label)
        a, b = host.detect(), dev.detect()
        _same_results(a, b)
        found += b
    dev.close()
    store.close()
    return found


def test_l12_detectors_agree_and_match_the_restatement(tmp_path, ctx, oracle, l12):
    poses, labels, clouds = l12
    cfg = lc.LoopClosureConfig(yaw_guess=True, max_correspondence_distance=GATE, gicp_epsilon=EPS, information_sigma=0.05,
                               information_floor=(1.0, 10.0), **gr.L12_CONFIG)
    ctx.reset_profile()
    got = _host_and_store(ctx, clouds, labels, cfg)
    assert ctx.get_profile()["small_launches"] > 0
    backend = ref.GicpOracleBackend(EPS, GATE, oracle)
    want = gr.run_detector(yr.YawLoopClosureDetector(backend, gr.l12_config()), clouds, labels)
    stop, gate = backend.min_margins()
    assert stop >= 1e-9 and gate >= 1e-9
    assert len(got) == len(want) == len(backend.runs) == 13
    assert [_key(r) for r in got] == [(w.query_frame, w.match_frame, w.sector_shift, backend.run_of(w).pairs) for w in want]
    for a, b in zip(got, want):
        assert _bits([a.scan_context_distance]) == _bits([b.scan_context_distance])
        dt, dr = synth.pose_delta(np.asarray(a.transform), np.asarray(b.transform))
        assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD and abs(a.icp_fitness - b.icp_fitness) <= HIST_ATOL
        # each closure's edge weight: finite, symmetric, 6 x 6
        assert a.information.shape == (6, 6) and np.isfinite(a.information).all() and np.array_equal(a.information, a.information.T)
        # ... and the closure is the stand-alone small-form call of its pair from the shift's start, bit for bit
        q, m = labels.index(a.query_frame), labels.index(a.match_frame)
        res, _hist, info = ctx.align_gicp(clouds[q], clouds[m], capi.Context.make_config(30, 1e-6, initial_transform=lc.sc_shift_transform(a.sector_shift)),
                                          (EPS, GATE, True))
        assert np.array_equal(_bits(_T(res)), _bits(a.transform)) and _bits([res.final_error]) == _bits([a.icp_fitness])
        assert info.pairs == a.pairs and res.converged
    print("  L12 worst error from truth: %.4f m over %d closures" % (rr.l12_worst(got, poses, labels), len(got)))

    # the C++ mirror (tests/cpp/gicp_loop_demo.cpp): both detectors, one align_gicp and a batch of two, the same numbers
    from lidar_slam_from_scratch_amd import build
    exe = tmp_path / "gicp_loop_demo"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "gicp_loop_demo.cpp"), "-o", str(exe), build.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(build.LIB_PATH), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lamdhip64"])
    args = []
    for k, (c, label) in enumerate(zip(clouds, labels)):
        c.tofile(tmp_path / ("c%d.f64" % k))
        args += [str(label), str(tmp_path / ("c%d.f64" % k))]
    kw = gr.L12_CONFIG
    subprocess.check_call([str(exe), str(tmp_path / "o.f64"), str(kw["frame_gap"]), repr(kw["sc_distance_threshold"]),
                           repr(kw["icp_fitness_threshold"]), str(kw["max_candidates"]), "1", repr(GATE), repr(EPS)] + args)
    o = np.fromfile(tmp_path / "o.f64")
    p = 0
    for _detector in ("host", "store"):
        assert int(o[p]) == len(got)
        p += 1
        for w in got:
            assert tuple(int(v) for v in o[p:p + 4]) == _key(w)
            assert o[p + 4] == w.scan_context_distance and o[p + 5] == w.icp_fitness
            assert (o[p + 6:p + 22].reshape(4, 4) == np.asarray(w.transform).reshape(4, 4)).all()
            p += 22
    res, _hist, info = ctx.align_gicp(clouds[-1], clouds[0], capi.Context.make_config(30), (EPS, GATE, True))
    for _call_no in range(3):                            # align_gicp, then the batch's two
        assert (int(o[p]), int(o[p + 1]), int(o[p + 2]), int(o[p + 3])) == (info.pairs, clouds[-1].shape[0], res.converged, res.num_iterations)
        assert o[p + 4] == res.final_error and (o[p + 5:p + 21].reshape(4, 4) == _T(res)).all()
        p += 21
    assert p == o.size


def test_set_gicp_zero_restores_the_gated_results(ctx, l12):
    _, labels, clouds = l12

    def run(switch_off_at):
        store = GlobalMap(ctx)
        cfg = lc.LoopClosureConfig(yaw_guess=True, max_correspondence_distance=GATE, **gr.L12_CONFIG)
        det = lc.StoreLoopClosureDetector(ctx, store, cfg)
        if switch_off_at is not None:
            det.set_gicp(EPS)
        found = []
        for k, (cloud, label) in enumerate(zip(clouds, labels)):
            if k == switch_off_at:
                det.set_gicp(0.0)
            store.add_frame(cloud)
            det.add_frame(store.size()[0] - 1, label)
            found.append(det.detect())
        det.close()
        store.close()
        return found

    gated, switched = run(None), run(9)
    assert sum(len(f) for f in switched[:9]) > 0 and sum(len(f) for f in gated[9:]) > 0
    assert any(not np.array_equal(_bits(a.transform), _bits(b.transform)) for fa, fb in zip(gated[:9], switched[:9])
               for a, b in zip(fa, fb))                  # plane-to-plane was on ...
    for a, b in zip(gated[9:], switched[9:]):            # ... and off again: the gated run's results, bit for bit
        _same_results(a, b)


def test_plane_to_plane_without_a_gate_reports_the_pairs(ctx, l12):
    """icpmi_loop_last_pairs while plane-to-plane is on, gate or not: both detectors, a scan met again where it was taken"""
    cloud = l12[2][0]
    found = _host_and_store(ctx, [cloud, cloud], [0, 100], lc.LoopClosureConfig(gicp_epsilon=EPS))
    assert len(found) == 1 and found[0].pairs == cloud.shape[0]   # no gate: every row is kept


# ------------------------------------------------------------------------------------------------ the SLAM driver

def test_run_slam_finds_the_detectors_closures(ctx):
    """D78L, the drive tests/test_gpu_gated.py closes behind loop_gate: the node's closures are the ones a detector with the
    same configuration finds over the same scans, bit for bit"""
    frames = yr.scans(gr.d78l_lateral_drive())
    run = slam.run_slam(frames, ctx, loop_yaw_guess=True, loop_gate=GATE, loop_gicp=EPS)
    cfg = slam.node_loop_config()
    cfg.yaw_guess, cfg.max_correspondence_distance, cfg.gicp_epsilon = True, GATE, EPS
    det = lc.LoopClosureDetector(lc.GpuBackend(ctx), cfg)
    want = []
    for k in range(1, len(frames)):
        det.add_frame(np.ascontiguousarray(frames[k], dtype=np.float64), k)
        if k % 10 == 0 and k > 50:
            want += det.detect()
    assert any(c.query_frame - c.match_frame >= 50 and c.pairs > 0 for c in run.closures)
    _same_results(run.closures, want)
    with pytest.raises(ValueError):
        slam.run_slam(frames[:2], ctx, loop_gicp=EPS, loop_robust=(capi.ROBUST_HUBER, 0.1))


# ------------------------------------------------------------------------------------------------ error codes

def test_error_codes(ctx, fixtures):
    lib = capi.load_library()
    f = fixtures["sub_33_700"]
    src, tgt = f["source"], f["target"]
    cfg = capi.Context.make_config()
    store = GlobalMap(ctx)
    det = lc.StoreLoopClosureDetector(ctx, store)
    for bad in (-1e-300, -1.0, 1.0 + 1e-12, math.nan, math.inf, -math.inf):
        assert lib.icpmi_loop_set_gicp(det._h, bad) == capi.ERR_ARG, bad
    assert lib.icpmi_loop_set_gicp(None, EPS) == capi.ERR_NULL
    assert lib.icpmi_loop_set_gicp(det._h, 1.0) == capi.OK and lib.icpmi_loop_set_gicp(det._h, 0.0) == capi.OK
    # plane-to-plane and robust weights exclude each other, in either order, and the refused setter changes nothing
    assert lib.icpmi_loop_set_gicp(det._h, EPS) == capi.OK
    assert lib.icpmi_loop_set_robust(det._h, capi.ROBUST_HUBER, 0.1) == capi.ERR_ARG
    assert lib.icpmi_loop_set_robust(det._h, 0, 0.0) == capi.OK              # (off is always taken)
    assert lib.icpmi_loop_set_gicp(det._h, 0.0) == capi.OK
    assert lib.icpmi_loop_set_robust(det._h, capi.ROBUST_HUBER, 0.1) == capi.OK   # the refused call had not left plane-to-plane half on
    assert lib.icpmi_loop_set_gicp(det._h, EPS) == capi.ERR_ARG
    assert lib.icpmi_loop_set_robust(det._h, 0, 0.0) == capi.OK
    assert lib.icpmi_loop_set_gicp(det._h, EPS) == capi.OK                   # ... nor the weights
    det.close()
    with pytest.raises(capi.IcpError) as e:
        lc.StoreLoopClosureDetector(ctx, store, lc.LoopClosureConfig(gicp_epsilon=EPS, robust_kind=capi.ROBUST_HUBER, robust_scale=0.1))
    assert e.value.code == capi.ERR_ARG
    store.close()
    host = lc.LoopClosureDetector(lc.GpuBackend(ctx), lc.LoopClosureConfig(gicp_epsilon=EPS, robust_kind=capi.ROBUST_HUBER, robust_scale=0.1))
    host.add_frame(src, 0)
    host.add_frame(src, 100)
    with pytest.raises(ValueError):
        host.detect()
    with pytest.raises(ValueError):
        lc.GpuBackend(ctx).align_many(src, [tgt], 30, 1e-6, gicp=(EPS,), robust=(capi.ROBUST_HUBER, 0.1))

    # the batch: NULL arrays, a bad count
    k = 2
    dpp = C.POINTER(C.c_double)
    sp, tp = (dpp * k)(capi._dp(src), capi._dp(src)), (dpp * k)(capi._dp(tgt), capi._dp(tgt))
    ns, nt = (C.c_int64 * k)(33, 33), (C.c_int64 * k)(700, 700)
    cfgs, rules = (capi.Config * k)(cfg, cfg), (capi.Gicp * k)(capi.as_gicp((EPS, 0.0, True)), capi.as_gicp((EPS,)))
    res, infos, status = (capi.Result * k)(), (capi.GicpInfo * k)(), (C.c_int32 * k)()
    hist = np.zeros((k, 51))
    good = [ctx._h, k, sp, ns, tp, nt, cfgs, rules, res, infos, capi._dp(hist), 51, status]
    assert lib.icpmi_align_gicp_batch(*good) == capi.OK and res[0].converged and res[1].converged
    for hole in (2, 3, 4, 5, 6, 7, 8, 10, 12):
        args = list(good)
        args[hole] = None
        assert lib.icpmi_align_gicp_batch(*args) == capi.ERR_NULL, hole
    args = list(good)
    args[9] = None                                       # infos may be NULL
    assert lib.icpmi_align_gicp_batch(*args) == capi.OK
    for count in (0, -1, lc.MAX_BATCH + 1):
        args = list(good)
        args[1] = count
        assert lib.icpmi_align_gicp_batch(*args) == capi.ERR_ARG, count
    assert lib.icpmi_align_gicp_batch(None, *good[1:]) == capi.ERR_NULL
    rules[1].epsilon = 0.0                               # a bad rule fails its problem, and the call
    assert lib.icpmi_align_gicp_batch(*good) == capi.ERR_ARG and status[0] == capi.OK and status[1] == capi.ERR_ARG
    # a context with a communicator (the callbacks form, one rank) runs neither form
    c = capi.Context(device=0)
    c.comm_init_callbacks(1, 0, lambda buf: None, lambda buf, per: None)
    with pytest.raises(capi.IcpError) as e:
        c.align_gicp(src, tgt, cfg, (EPS, 0.0, True))
    assert e.value.code == capi.ERR_ARG
    with pytest.raises(capi.IcpError) as e:
        c.align_gicp_batch([src], [tgt], cfg, (EPS, 0.0, True))
    assert e.value.code == capi.ERR_ARG
    c.comm_finalize()
    res, _hist, info = c.align_gicp(src, tgt, cfg, (EPS, 0.0, True))   # and does again without one
    assert res.converged and info.pairs == 33
    c.close()
