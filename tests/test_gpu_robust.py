"""Robust row weights on the device: k_icp_small_robust, k_reduce_robust and k_finish_step_robust behind
icpmi_align_robust / _device / _batch, icpmi_loop_set_robust and icpmi_stream_set_robust.  A Huber scale above every
residual gives the unweighted call's bits on both paths, and behind a gate the gated call's; at Huber 0.1 m and
Geman-McClure 0.3 m the calls agree with the CPU restatement (scripts/robust_icp_ref.py) within tests/test_gpu_parity.py's
tolerances, keep the same rows and sum the same weights; dropped rows, a pass without pairs, row counts around the small
kernel's 32-row blocks and one to five kept rows; the batch; the three detectors on L12; the stream against
icpmi_align_robust on the same filtered scans; the node's loop and the stream's driver; the error codes."""
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
import loop_yaw_ref as yr  # noqa: E402
import robust_icp_ref as ref  # noqa: E402
from lidar_slam_from_scratch_amd import capi, odometry, synth  # noqa: E402
from lidar_slam_from_scratch_amd import loop_closure as lc  # noqa: E402
from lidar_slam_from_scratch_amd import slam  # noqa: E402
from lidar_slam_from_scratch_amd.global_map import GlobalMap  # noqa: E402

pytestmark = pytest.mark.gpu

POSE_TOL_M, POSE_TOL_RAD, HIST_ATOL = 1e-4, 1e-4, 1e-9   # tests/test_gpu_parity.py's
WEIGHT_RTOL = 1e-9
GATE = gr.L12_GATE
HUBER, GM = (capi.ROBUST_HUBER, ref.HUBER_SCALE), (capi.ROBUST_GEMAN_MCCLURE, ref.GM_SCALE)
RULES = {"huber": HUBER, "gm": GM}
ALL = (capi.ROBUST_HUBER, 1e30)                          # a Huber scale above every |b|: every weight is 1.0
ENGINES = {"auto": capi.SEARCH_AUTO, "exact_f64": capi.SEARCH_EXACT_F64, "mfma_bf16": capi.SEARCH_MFMA_BF16,
           "mfma_pruned": capi.SEARCH_MFMA_PRUNED}
DRIVE_FRAMES = 12


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
def l12():
    return gr.l12_scans()


@pytest.fixture(scope="module")
def cases(oracle, l12):
    """name -> (source, target, start, gate, max_iterations, {rule: the restatement's result}, small path on the default
    context?), once"""
    pairs = {}
    for q, m in gr.L12_PAIRS:
        s, t, start = gr.l12_pair(l12[2], q, m, oracle)
        pairs["l12_%d_%d" % (q, m)] = (s, t, start, GATE, 30, True)
    s, t, _ = synth.c2_lidar_pair()
    pairs["c2"] = (s, t, None, 0.0, 50, True)
    s, t = gr.general_pair()
    pairs["general_700_17000"] = (s, t, None, GATE, 30, False)
    out = {}
    for name, (s, t, start, gate, max_it, small) in pairs.items():
        tree = oracle.KDTree(t)
        nrm = oracle.estimate_normals(t, tree, 20)
        want = {rule: ref.robust_icp(s, t, k, scale, gate, max_it, 1e-6, 1e-9, start, orc=oracle, normals=nrm, tree=tree)
                for rule, (k, scale) in RULES.items()}
        out[name] = (s, t, start, gate, max_it, want, small)
    return out


@pytest.fixture(scope="module")
def drive():
    """-> (raw scans, filtered frames, true poses) of frames 0..11 of the default drive: tests/test_robust_reference.py's"""
    raw = [synth.lidar_frame(f, voxel=0) for f in range(DRIVE_FRAMES)]
    return raw, [synth.voxel_centroids(r, 0.5) for r in raw], [synth.lidar_pose(f) for f in range(DRIVE_FRAMES)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _T(res):
    return np.array(res.transformation[:]).reshape(4, 4)


def _same_bits(a, b):
    """two (Result, history, ...) outcomes"""
    assert np.array_equal(_bits(_T(a[0])), _bits(_T(b[0])))
    assert np.array_equal(_bits(a[1]), _bits(b[1]))
    assert (a[0].converged, a[0].num_iterations, a[0].history_len, a[0].loop_iterations) == \
        (b[0].converged, b[0].num_iterations, b[0].history_len, b[0].loop_iterations)
    assert _bits([a[0].final_error]) == _bits([b[0].final_error])


def _same_info(a, b):
    assert (a.pairs, a.rows) == (b.pairs, b.rows) and _bits([a.weight_sum]) == _bits([b.weight_sum])


def _ran(c, call):
    """-> (the call's outcome, iterations it ran in the small-cloud kernel)"""
    c.reset_profile()
    out = call()
    return out, c.get_profile()["small_launches"]


def _room(n_src, n_tgt):
    return synth.c1_room_corner(n_src)[0], synth.c1_room_corner(n_tgt)[1]


# ------------------------------------------------------------------------------------------------ every weight 1.0

@pytest.mark.parametrize("n_tgt", [1500, 4500])          # one split; three splits, the last ragged
def test_unit_weights_small_kernel_bit_for_bit(ctx, n_tgt):
    src, tgt = _room(1001, n_tgt)                        # 1,001 rows: no multiple of the kernel's 32
    cfg = capi.Context.make_config()
    want, small_w = _ran(ctx, lambda: ctx.align(src, tgt, cfg))
    got, small_g = _ran(ctx, lambda: ctx.align_robust(src, tgt, cfg, ALL))
    assert small_w > 0 and small_g == small_w            # both ran in the small-cloud kernel
    _same_bits(got, want)
    assert (got[2].pairs, got[2].rows, got[2].weight_sum) == (1001, 1001, 1001.0) and want[0].converged
    gated = ctx.align_gated(src, tgt, cfg, GATE)
    got, small_g = _ran(ctx, lambda: ctx.align_robust(src, tgt, cfg, ALL + (GATE,)))
    assert small_g > 0
    _same_bits(got, gated)
    assert got[2].pairs == gated[2] and got[2].weight_sum == float(gated[2])


@pytest.mark.parametrize("n_src,n_tgt", [(300, 700), (5000, 5000)])
def test_unit_weights_general_path_bit_for_bit(contexts, n_src, n_tgt):
    c = contexts("exact_f64")
    src, tgt = _room(n_src, n_tgt)
    cfg = capi.Context.make_config()
    want, small_w = _ran(c, lambda: c.align(src, tgt, cfg))
    got, small_g = _ran(c, lambda: c.align_robust(src, tgt, cfg, ALL))
    assert small_w == 0 and small_g == 0
    _same_bits(got, want)
    assert (got[2].pairs, got[2].weight_sum) == (n_src, float(n_src)) and want[0].converged
    gated = c.align_gated(src, tgt, cfg, GATE)
    got, small_g = _ran(c, lambda: c.align_robust(src, tgt, cfg, ALL + (GATE,)))
    assert small_g == 0
    _same_bits(got, gated)
    assert got[2].pairs == gated[2] and got[2].weight_sum == float(gated[2])


# ------------------------------------------------------------------------------------------------ the restatement

def _against_restatement(got, want):
    res, hist, info = got
    dt, dr = synth.pose_delta(_T(res), want.transformation)
    print("  %.3e m %.3e rad, history differs by %.3e, pairs %d / %d, weight sum differs by %.3e of %.6f, iterations %d / %d"
          % (dt, dr, np.abs(hist - want.error_history).max() if len(hist) == len(want.error_history) else math.nan,
             info.pairs, want.pairs, abs(info.weight_sum - want.weight_sum), want.weight_sum, res.num_iterations,
             want.num_iterations))
    assert res.num_iterations == want.num_iterations and bool(res.converged) == want.converged
    assert info.pairs == want.pairs
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD
    assert np.allclose(hist, want.error_history, rtol=0.0, atol=HIST_ATOL)
    assert abs(res.final_error - want.final_error) <= HIST_ATOL
    assert abs(info.weight_sum - want.weight_sum) <= WEIGHT_RTOL * want.weight_sum


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("case", ["l12_8_3", "l12_6_5", "c2", "general_700_17000"])
def test_parity_with_the_restatement(contexts, cases, case, rule, engine):
    c = contexts(engine)
    src, tgt, start, gate, max_it, wants, small_by_default = cases[case]
    want = wants[rule]
    assert want.converged and 0.0 < want.weight_sum < want.pairs <= src.shape[0]      # rows are down-weighted
    assert (want.pairs < src.shape[0]) == (gate > 0.0)                                 # and, behind a gate, dropped
    cfg = capi.Context.make_config(max_iterations=max_it, tolerance=1e-6, initial_transform=start)
    got, small = _ran(c, lambda: c.align_robust(src, tgt, cfg, RULES[rule] + (gate,)))
    if engine == "auto":                                 # the two paths, on the default context
        assert (small > 0) == small_by_default
    assert got[2].rows == src.shape[0]
    _against_restatement(got, want)


# ------------------------------------------------------------------------------------------------ edges

@pytest.mark.parametrize("engine,n_src,n_tgt", [("auto", 1001, 1500), ("exact_f64", 300, 700)])
def test_a_row_of_nans_is_dropped(contexts, engine, n_src, n_tgt):
    """with no gate given (g2 = DBL_MAX) too.  The row is the last, so every other row keeps its thread and its place in
    the sums: on the exact engine the bits are those of the call without it."""
    c = contexts(engine)
    src, tgt = _room(n_src, n_tgt)
    bad = np.vstack([src, [[math.nan] * 3]])
    cfg = capi.Context.make_config()
    for rule in (HUBER, GM + (GATE,)):
        got, small = _ran(c, lambda: c.align_robust(bad, tgt, cfg, rule))
        assert (small > 0) == (engine == "auto")
        want = c.align_robust(src, tgt, cfg, rule)
        assert got[2].pairs == want[2].pairs and got[2].rows == n_src + 1
        assert got[2].pairs == n_src or len(rule) == 3    # n - 1 of the n rows handed in, where no gate drops more
        assert got[0].converged == want[0].converged == 1
        if engine == "exact_f64":
            _same_bits(got, want)
            assert _bits([got[2].weight_sum]) == _bits([want[2].weight_sum])
        else:
            dt, dr = synth.pose_delta(_T(got[0]), _T(want[0]))
            assert got[0].num_iterations == want[0].num_iterations and dt <= POSE_TOL_M and dr <= POSE_TOL_RAD
            assert np.allclose(got[1], want[1], rtol=0.0, atol=HIST_ATOL)
    inf = np.vstack([src, [[math.inf, 0.0, 0.0]]])                 # an infinite row: d2 = +Inf is above DBL_MAX
    res, _hist, info = c.align_robust(inf, tgt, cfg, HUBER)
    assert info.pairs == n_src and res.converged


@pytest.mark.parametrize("engine,n_src,n_tgt", [("auto", 1001, 1500), ("exact_f64", 300, 700)])
def test_no_pairs_ends_the_call(contexts, engine, n_src, n_tgt):
    c = contexts(engine)
    src, tgt = _room(n_src, n_tgt)
    far = src + np.array([100.0, 0.0, 0.0])
    (res, hist, info), small = _ran(c, lambda: c.align_robust(far, tgt, capi.Context.make_config(), HUBER + (1.0,)))
    assert (small > 0) == (engine == "auto")
    assert hist.tolist() == [math.inf, math.inf] and res.final_error == math.inf
    assert not res.converged and res.num_iterations == 1 and res.loop_iterations == 1
    assert info.pairs == 0 and info.weight_sum == 0.0 and info.rows == n_src
    assert np.array_equal(_T(res), np.eye(4))
    # the post-loop pass alone (no iterations asked for) enters +Inf once
    res, hist, info = c.align_robust(far, tgt, capi.Context.make_config(max_iterations=0), GM + (1.0,))
    assert hist.tolist() == [math.inf] and res.num_iterations == 0 and not res.converged
    assert info.pairs == 0 and info.weight_sum == 0.0
    # and the context goes on as before
    res, _hist, info = c.align_robust(src, tgt, capi.Context.make_config(), HUBER + (5.0,))
    assert res.converged and info.pairs == n_src and 0.0 < info.weight_sum <= n_src


@pytest.mark.parametrize("n_src", [1, 31, 33, 1001])
def test_row_counts_around_the_small_kernels_blocks(contexts, oracle, n_src):
    """the small kernel's blocks take 32 rows: one row, a block short of one, a block and one row, 31 blocks and nine"""
    ctx, exact = contexts("mfma_bf16"), contexts("exact_f64")    # (AUTO takes the exact engine below 64 rows)
    src, tgt = _room(1001, 1500)
    src = np.ascontiguousarray(src[:n_src])
    cfg = capi.Context.make_config(max_iterations=10)
    got, small = _ran(ctx, lambda: ctx.align_robust(src, tgt, cfg, HUBER))
    assert small > 0
    want = exact.align_robust(src, tgt, cfg, HUBER)                      # the general path's kernels, the same sums
    assert got[2].pairs == want[2].pairs == n_src and got[0].num_iterations == want[0].num_iterations
    assert abs(got[2].weight_sum - want[2].weight_sum) <= WEIGHT_RTOL * want[2].weight_sum
    assert np.allclose(got[1], want[1], rtol=0.0, atol=HIST_ATOL) and np.isfinite(got[1]).all()
    assert np.isfinite(_T(got[0])).all()
    if n_src >= 31:                                      # (below six rows the solve is rank-deficient: the zero-pivot rule)
        dt, dr = synth.pose_delta(_T(got[0]), _T(want[0]))
        assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD


@pytest.mark.parametrize("engine", ["mfma_bf16", "exact_f64"])
def test_one_to_five_kept_rows_go_through_the_zero_pivot_rule(contexts, engine):
    """fewer kept rows than unknowns: the 6 x 6 system is singular, the pivoted LDLT's zero-pivot rule answers, and the
    call ends with finite numbers on both paths"""
    c = contexts(engine)
    src, tgt = _room(1001, 1500)
    for kept in range(1, 6):
        far = src[:40] + np.array([100.0, 0.0, 0.0])
        far[:kept] = tgt[:kept] + 0.01                   # `kept` rows on the target, the rest 100 m away behind a 2 m gate
        for rule in (HUBER, GM):
            res, hist, info = c.align_robust(far, tgt, capi.Context.make_config(max_iterations=0), rule + (GATE,))
            assert info.pairs == kept and 0.0 < info.weight_sum <= kept and len(hist) == 1 and math.isfinite(hist[0])
            (res, hist, info), small = _ran(c, lambda: c.align_robust(far, tgt, capi.Context.make_config(max_iterations=5), rule + (GATE,)))
            assert (small > 0) == (engine == "mfma_bf16")    # (40 rows: AUTO would take the exact engine)
            assert 0 <= info.pairs <= 40 and 0.0 <= info.weight_sum <= info.pairs
            assert res.history_len == len(hist) >= 1 and not np.isnan(hist).any()
            assert np.isfinite(_T(res)).all()


# ------------------------------------------------------------------------------------------------ batch, device pointers

def test_batch_is_the_sequential_calls_bit_for_bit(ctx, cases):
    s1, t1, start, _, _, _, _ = cases["l12_8_3"]
    s2, t2 = _room(1001, 4500)
    s3, t3 = _room(300, 700)
    srcs, tgts = [s1, s2, s3 + np.array([0.0, 100.0, 0.0])], [t1, t2, t3]
    cfgs = [capi.Context.make_config(30, 1e-6, initial_transform=start), capi.Context.make_config(), capi.Context.make_config(20)]
    rules = [HUBER + (GATE,), GM, (capi.ROBUST_HUBER, 0.05, 1.0)]
    alone = [ctx.align_robust(s, t, k, r) for s, t, k, r in zip(srcs, tgts, cfgs, rules)]
    together = ctx.align_robust_batch(srcs, tgts, cfgs, rules)
    for a, b in zip(alone, together):
        _same_bits(a, b)
        _same_info(a[2], b[2])
    assert together[2][2].pairs == 0 and together[2][1].tolist() == [math.inf, math.inf]
    assert 0 < together[0][2].pairs < s1.shape[0] and together[1][2].pairs == 1001
    assert 0.0 < together[1][2].weight_sum < 1001.0


def test_device_pointers_give_the_host_call(ctx, cases):
    src, tgt, start, _, _, _, _ = cases["l12_6_5"]
    cfg = capi.Context.make_config(30, 1e-6, initial_transform=start)
    ds, dt_ = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    torch.cuda.synchronize()
    got = ctx.align_robust_device(ds.data_ptr(), src.shape[0], dt_.data_ptr(), tgt.shape[0], cfg, GM + (GATE,))
    want = ctx.align_robust(src, tgt, cfg, GM + (GATE,))
    _same_bits(got, want)
    _same_info(got[2], want[2])


# ------------------------------------------------------------------------------------------------ the detectors

def _key(r):
    return (r.query_frame, r.match_frame, r.sector_shift, r.pairs)


def _same_results(a, b):
    assert [_key(r) for r in a] == [_key(r) for r in b]
    for x, y in zip(a, b):
        assert (x.weight_sum is None) == (y.weight_sum is None)
        assert x.weight_sum is None or _bits([x.weight_sum]) == _bits([y.weight_sum])
        assert _bits([x.scan_context_distance]) == _bits([y.scan_context_distance])
        assert _bits([x.icp_fitness]) == _bits([y.icp_fitness])
        assert np.array_equal(_bits(x.transform), _bits(y.transform))


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


def _l12_cfg(kind, scale):
    return lc.LoopClosureConfig(yaw_guess=True, max_correspondence_distance=GATE, robust_kind=kind, robust_scale=scale,
                                **gr.L12_CONFIG)


def test_l12_detectors_agree_and_match_the_restatement(tmp_path, ctx, oracle, l12):
    poses, labels, clouds = l12
    got = _host_and_store(ctx, clouds, labels, _l12_cfg(*HUBER))
    backend = ref.RobustOracleBackend(ref.HUBER, ref.HUBER_SCALE, GATE, oracle)
    want = gr.run_detector(yr.YawLoopClosureDetector(backend, gr.l12_config()), clouds, labels)
    stop, gate = backend.min_margins()
    assert stop >= 1e-9 and gate >= 1e-9
    assert {r.query_frame for r in got} == set(range(100, 106)) and len(got) == len(want) == 13
    assert [_key(r) for r in got] == [(w.query_frame, w.match_frame, w.sector_shift, backend.run_of(w).pairs) for w in want]
    for a, b in zip(got, want):
        run = backend.run_of(b)
        assert _bits([a.scan_context_distance]) == _bits([b.scan_context_distance])
        dt, dr = synth.pose_delta(np.asarray(a.transform), np.asarray(b.transform))
        assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD and abs(a.icp_fitness - b.icp_fitness) <= HIST_ATOL
        assert abs(a.weight_sum - run.weight_sum) <= WEIGHT_RTOL * run.weight_sum
    print("  L12 worst error from truth: %.4f m over %d closures" % (ref.l12_worst(got, poses, labels), len(got)))

    # the C++ mirror (tests/cpp/robust_demo.cpp): both detectors and one align_robust, the same numbers
    from lidar_slam_from_scratch_amd import build
    exe = tmp_path / "robust_demo"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "robust_demo.cpp"), "-o", str(exe), build.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(build.LIB_PATH), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lamdhip64"])
    args = []
    for k, (c, label) in enumerate(zip(clouds, labels)):
        c.tofile(tmp_path / ("c%d.f64" % k))
        args += [str(label), str(tmp_path / ("c%d.f64" % k))]
    kw = gr.L12_CONFIG
    subprocess.check_call([str(exe), str(tmp_path / "o.f64"), str(kw["frame_gap"]), repr(kw["sc_distance_threshold"]),
                           repr(kw["icp_fitness_threshold"]), str(kw["max_candidates"]), "1", repr(GATE),
                           str(HUBER[0]), repr(HUBER[1])] + args)
    o = np.fromfile(tmp_path / "o.f64")
    p = 0
    for _detector in ("host", "store"):
        assert int(o[p]) == len(got)
        p += 1
        for w in got:
            assert tuple(int(v) for v in o[p:p + 4]) == _key(w)
            assert o[p + 4] == w.weight_sum and o[p + 5] == w.scan_context_distance and o[p + 6] == w.icp_fitness
            assert (o[p + 7:p + 23].reshape(4, 4) == np.asarray(w.transform).reshape(4, 4)).all()
            p += 23
    res, _hist, info = ctx.align_robust(clouds[-1], clouds[0], capi.Context.make_config(30), HUBER + (GATE,))
    assert o[p] == info.weight_sum
    assert (int(o[p + 1]), int(o[p + 2]), int(o[p + 3]), int(o[p + 4])) == (info.pairs, clouds[-1].shape[0], res.converged, res.num_iterations)
    assert o[p + 5] == res.final_error and (o[p + 6:p + 22].reshape(4, 4) == _T(res)).all()
    assert p + 22 == o.size


def test_set_robust_zero_restores_the_gated_results(ctx, l12):
    _, labels, clouds = l12

    def run(switch_off_at):
        store = GlobalMap(ctx)
        cfg = lc.LoopClosureConfig(yaw_guess=True, max_correspondence_distance=GATE, **gr.L12_CONFIG)
        det = lc.StoreLoopClosureDetector(ctx, store, cfg)
        if switch_off_at is not None:
            det.set_robust(*GM)
        found = []
        for k, (cloud, label) in enumerate(zip(clouds, labels)):
            if k == switch_off_at:
                det.set_robust(0, 0.0)
            store.add_frame(cloud)
            det.add_frame(store.size()[0] - 1, label)
            found.append(det.detect())
        det.close()
        store.close()
        return found

    gated, switched = run(None), run(9)
    assert any(r.weight_sum is not None and 0.0 < r.weight_sum < r.pairs for f in switched[:9] for r in f)   # the weights were on ...
    assert sum(len(f) for f in gated[9:]) > 0
    for a, b in zip(gated[9:], switched[9:]):            # ... and off again: the gated run's results, bit for bit
        assert all(r.weight_sum is None for r in b)
        _same_results(a, b)
    lib = capi.load_library()
    store = GlobalMap(ctx)
    det = lc.StoreLoopClosureDetector(ctx, store)
    for kind, scale in ((3, 0.1), (-1, 0.1), (1, 0.0), (1, -1.0), (2, math.nan), (2, math.inf)):
        assert lib.icpmi_loop_set_robust(det._h, kind, scale) == capi.ERR_ARG
    assert lib.icpmi_loop_set_robust(None, 1, 0.1) == capi.ERR_NULL
    assert lib.icpmi_loop_set_robust(det._h, 0, math.nan) == capi.OK       # kind 0 is off, whatever the scale
    n = C.c_int64(-1)
    assert lib.icpmi_loop_last_weights(det._h, None, 0, C.byref(n)) == capi.OK and n.value == 0
    det.close()
    store.close()


# ------------------------------------------------------------------------------------------------ the stream

def _write_bins(tmp_path, raw):
    paths = []
    for k, r in enumerate(raw):
        rec = np.zeros((r.shape[0], 4), dtype=np.float32)
        rec[:, :3] = r
        path = tmp_path / ("%06d.bin" % k)
        path.write_bytes(rec.tobytes())
        paths.append(str(path))
    return paths


def test_stream_registers_under_the_rule(tmp_path, ctx, drive):
    """every push equals icpmi_align_robust on the same filtered scans bit for bit -- the targets are the ones prepared on
    the helper context during the previous push and adopted; stream_last_robust; NULL restores the plain stream; with the
    prefetch worker the same"""
    raw = drive[0]
    paths = _write_bins(tmp_path, raw)
    cfg = capi.Context.make_config()
    rule = HUBER + (GATE,)
    stream = capi.Context(device=0)
    try:
        stream.stream_set_robust(rule)
        prev, registered = None, []
        for k, p in enumerate(paths):
            res, hist, info = stream.stream_push_file(p, 0.5, 1000, cfg)
            cur = stream.stream_current_scan()
            last = stream.stream_last_robust()
            if k == 0:
                assert info.status == capi.STREAM_FIRST_FRAME and (last.weight_sum, last.pairs, last.rows) == (0.0, 0, 0)
            else:
                assert info.status == capi.STREAM_REGISTERED
                want = ctx.align_robust(cur, prev, cfg, rule)
                _same_bits((res, hist), want)
                _same_info(last, want[2])
                assert 0.0 < last.weight_sum < last.pairs <= last.rows == cur.shape[0]
                registered.append((res, hist, last.weight_sum))
            prev = cur
        # the drivers: with and without the prefetch worker, the same registrations
        a = odometry.run_odometry_stream(paths, stream, prefetch=False, robust=rule)
        b = odometry.run_odometry_stream(paths, stream, prefetch=True, robust=rule)
        for t in (a, b):
            assert t.iterations == [r.num_iterations for r, _, _ in registered]
            assert np.array_equal(_bits(t.final_errors), _bits([r.final_error for r, _, _ in registered]))
            assert np.array_equal(_bits(t.weight_sums), _bits([w for _, _, w in registered]))
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a.poses, b.poses))
        # NULL: the plain stream's bits again
        off = odometry.run_odometry_stream(paths[:5], stream, prefetch=False)
        last = stream.stream_last_robust()
        assert (last.weight_sum, last.pairs, last.rows) == (0.0, 0, 0) and off.weight_sums == []
    finally:
        stream.close()
    fresh = capi.Context(device=0)
    try:
        plain = odometry.run_odometry_stream(paths[:5], fresh, prefetch=False)
    finally:
        fresh.close()
    assert off.iterations == plain.iterations and np.array_equal(_bits(off.final_errors), _bits(plain.final_errors))
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(off.poses, plain.poses))
    assert not np.array_equal(_bits(off.final_errors), _bits(a.final_errors[:4]))   # (and the rule did change the registrations)


def test_robust_odometry_drifts_less(tmp_path, ctx, drive):
    """tests/test_robust_reference.py's drive through slam.run_slam and odometry.run_odometry_stream, both on the GPU:
    the ordering alone is asserted, DESIGN 7.10 records the numbers"""
    raw, frames, poses = drive

    class _Track:
        pass

    def ate(run_poses):
        t = _Track()
        t.poses = run_poses
        return odometry.absolute_trajectory_error(t, poses)

    plain = slam.run_slam(frames, ctx)
    robust = slam.run_slam(frames, ctx, odom_robust=HUBER, loop_robust=HUBER)
    print("  run_slam ATE rms: plain %.3f m, Huber %.3f m" % (ate(plain.poses), ate(robust.poses)))
    assert len(robust.poses) == len(plain.poses) == DRIVE_FRAMES and ate(robust.poses) < ate(plain.poses)
    with pytest.raises(ValueError):
        slam.run_slam(frames[:2], ctx, align=odometry.gpu_align(ctx), odom_robust=HUBER)
    paths = _write_bins(tmp_path, raw)
    stream = capi.Context(device=0)
    try:
        s_plain = odometry.run_odometry_stream(paths, stream)
        s_robust = odometry.run_odometry_stream(paths, stream, robust=HUBER)
    finally:
        stream.close()
    print("  run_odometry_stream ATE rms: plain %.3f m, Huber %.3f m" % (ate(s_plain.poses), ate(s_robust.poses)))
    assert ate(s_robust.poses) < ate(s_plain.poses) and len(s_robust.weight_sums) == DRIVE_FRAMES - 1


# ------------------------------------------------------------------------------------------------ error codes

def test_error_codes(ctx):
    lib = capi.load_library()
    src, tgt = _room(300, 700)
    cfg = capi.Context.make_config()
    bad_rules = [(3, 0.1), (0, 0.1), (-1, 0.1), (1, 0.0), (1, -0.1), (2, math.nan), (2, math.inf), (1, -math.inf),
                 (1, 0.1, -2.0), (2, 0.3, math.nan), (1, 0.1, math.inf)]
    for bad in bad_rules:
        with pytest.raises(capi.IcpError) as e:
            ctx.align_robust(src, tgt, cfg, bad)
        assert e.value.code == capi.ERR_ARG, bad
        with pytest.raises(capi.IcpError) as e:
            ctx.align_robust_batch([src], [tgt], cfg, bad)
        assert e.value.code == capi.ERR_ARG, bad
        with pytest.raises(capi.IcpError) as e:
            ctx.stream_set_robust(bad)
        assert e.value.code == capi.ERR_ARG, bad
    hist, res = np.zeros(51), capi.Result()
    assert lib.icpmi_align_robust(ctx._h, capi._dp(src), 300, capi._dp(tgt), 700, C.byref(cfg), None, C.byref(res), None,
                                  capi._dp(hist), 51) == capi.ERR_NULL     # no rule: that is icpmi_align
    rule = capi.as_robust(HUBER)
    assert lib.icpmi_align_robust(ctx._h, capi._dp(src), 300, capi._dp(tgt), 700, C.byref(cfg), C.byref(rule), C.byref(res),
                                  None, capi._dp(hist), 51) == capi.OK     # info may be NULL
    assert lib.icpmi_align_robust(ctx._h, capi._dp(src), 300, capi._dp(tgt), 700, C.byref(cfg), C.byref(rule), C.byref(res),
                                  None, capi._dp(hist), 50) == capi.ERR_CAPACITY
    assert lib.icpmi_stream_last_robust(ctx._h, None) == capi.ERR_NULL
    # a context with a communicator (the callbacks form, one rank) does not run robust registrations
    c = capi.Context(device=0)
    c.comm_init_callbacks(1, 0, lambda buf: None, lambda buf, per: None)
    with pytest.raises(capi.IcpError) as e:
        c.align_robust(src, tgt, cfg, HUBER)
    assert e.value.code == capi.ERR_ARG
    with pytest.raises(capi.IcpError) as e:
        c.align_robust_batch([src], [tgt], cfg, HUBER)
    assert e.value.code == capi.ERR_ARG
    with pytest.raises(capi.IcpError) as e:
        c.stream_set_robust(HUBER)
    assert e.value.code == capi.ERR_ARG
    c.comm_finalize()
    res, _hist, info = c.align_robust(src, tgt, cfg, HUBER)            # and does again without one
    assert res.converged and info.pairs == 300
    c.close()
