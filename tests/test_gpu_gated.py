"""The correspondence-distance gate on the device: k_icp_small_gated, k_reduce_gated and
k_finish_step_gated behind icpmi_align_gated / _device / _batch and icpmi_loop_set_gate.  A gate that keeps every row
gives the ungated call's bits on both paths; at 2 m the calls agree with the CPU restatement (scripts/gated_icp_ref.py)
within tests/test_gpu_parity.py's tolerances and keep the same rows; a row of NaNs is dropped; a pass without pairs ends
the call; the three detectors agree on L12 (R12 with the return leg 1.5 m aside) among themselves bit for bit and with
the restatement; the node's loop through slam.run_slam; the error codes."""
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

import gated_icp_ref as ref  # noqa: E402
import loop_yaw_ref as yr  # noqa: E402
from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402
from lidar_slam_from_scratch_amd import loop_closure as lc  # noqa: E402
from lidar_slam_from_scratch_amd import slam  # noqa: E402
from lidar_slam_from_scratch_amd.global_map import GlobalMap  # noqa: E402

pytestmark = pytest.mark.gpu

POSE_TOL_M, POSE_TOL_RAD, HIST_ATOL = 1e-4, 1e-4, 1e-9   # tests/test_gpu_parity.py's
GATE = ref.L12_GATE
ENGINES = {"auto": capi.SEARCH_AUTO, "exact_f64": capi.SEARCH_EXACT_F64, "mfma_bf16": capi.SEARCH_MFMA_BF16,
           "mfma_pruned": capi.SEARCH_MFMA_PRUNED}


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
    return ref.l12_scans()


@pytest.fixture(scope="module")
def cases(oracle, l12):
    """name -> (source, target, start, the restatement's result at GATE, small path on the default context?), once"""
    out = {}
    for q, m in ref.L12_PAIRS:
        s, t, start = ref.l12_pair(l12[2], q, m, oracle)
        out["l12_%d_%d" % (q, m)] = (s, t, start, ref.gated_icp(s, t, GATE, 30, 1e-6, 1e-9, start, orc=oracle), True)
    s, t = ref.general_pair()
    out["general_700_17000"] = (s, t, None, ref.gated_icp(s, t, GATE, 30, 1e-6, 1e-9, orc=oracle), False)
    return out


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


def _ran(c, call):
    """-> (the call's outcome, iterations it ran in the small-cloud kernel)"""
    c.reset_profile()
    out = call()
    return out, c.get_profile()["small_launches"]


def _room(n_src, n_tgt):
    return synth.c1_room_corner(n_src)[0], synth.c1_room_corner(n_tgt)[1]


# ------------------------------------------------------------------------------------------------ a gate that keeps all

@pytest.mark.parametrize("n_tgt", [1500, 4500])          # one split; three splits, the last ragged
def test_gate_keeps_all_small_kernel_bit_for_bit(ctx, n_tgt):
    src, tgt = _room(1001, n_tgt)                        # 1,001 rows: no multiple of the kernel's 32
    cfg = capi.Context.make_config()
    want, small_w = _ran(ctx, lambda: ctx.align(src, tgt, cfg))
    got, small_g = _ran(ctx, lambda: ctx.align_gated(src, tgt, cfg, 1e6))
    assert small_w > 0 and small_g == small_w            # both ran in the small-cloud kernel
    _same_bits(got, want)
    assert got[2] == 1001 and want[0].converged


@pytest.mark.parametrize("n_src,n_tgt", [(300, 700), (5000, 5000)])
def test_gate_keeps_all_general_path_bit_for_bit(contexts, n_src, n_tgt):
    c = contexts("exact_f64")
    src, tgt = _room(n_src, n_tgt)
    cfg = capi.Context.make_config()
    want, small_w = _ran(c, lambda: c.align(src, tgt, cfg))
    got, small_g = _ran(c, lambda: c.align_gated(src, tgt, cfg, 1e6))
    assert small_w == 0 and small_g == 0
    _same_bits(got, want)
    assert got[2] == n_src and want[0].converged


# ------------------------------------------------------------------------------------------------ the restatement

def _against_restatement(got, want):
    res, hist, pairs = got
    dt, dr = synth.pose_delta(_T(res), want.transformation)
    print("  %.3e m %.3e rad, history differs by %.3e, pairs %d / %d, iterations %d / %d"
          % (dt, dr, np.abs(hist - want.error_history).max() if len(hist) == len(want.error_history) else math.nan,
             pairs, want.pairs, res.num_iterations, want.num_iterations))
    assert res.num_iterations == want.num_iterations and bool(res.converged) == want.converged
    assert pairs == want.pairs
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD
    assert np.allclose(hist, want.error_history, rtol=0.0, atol=HIST_ATOL)
    assert abs(res.final_error - want.final_error) <= HIST_ATOL


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("case", ["l12_8_3", "l12_6_5", "general_700_17000"])
def test_parity_with_the_restatement(contexts, cases, case, engine):
    c = contexts(engine)
    src, tgt, start, want, small_by_default = cases[case]
    assert 0 < want.pairs < src.shape[0]                 # the gate drops rows, and not all
    cfg = capi.Context.make_config(max_iterations=30, tolerance=1e-6, initial_transform=start)
    got, small = _ran(c, lambda: c.align_gated(src, tgt, cfg, GATE))
    if engine == "auto":                                 # the two paths, on the default context
        assert (small > 0) == small_by_default
    _against_restatement(got, want)


# ------------------------------------------------------------------------------------------------ dropped rows, no pairs

@pytest.mark.parametrize("engine,n_src,n_tgt", [("auto", 1001, 1500), ("exact_f64", 300, 700)])
def test_a_row_of_nans_is_dropped(contexts, engine, n_src, n_tgt):
    c = contexts(engine)
    src, tgt = _room(n_src, n_tgt)
    bad = np.insert(src, n_src // 2, np.nan, axis=0)
    cfg = capi.Context.make_config()
    (res, hist, pairs), small = _ran(c, lambda: c.align_gated(bad, tgt, cfg, 1e6))
    assert (small > 0) == (engine == "auto")
    want = c.align_gated(src, tgt, cfg, 1e6)
    assert pairs == n_src and want[2] == n_src           # n - 1 of the n rows handed in
    dt, dr = synth.pose_delta(_T(res), _T(want[0]))
    assert res.num_iterations == want[0].num_iterations and res.converged == want[0].converged == 1
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD and np.allclose(hist, want[1], rtol=0.0, atol=HIST_ATOL)


@pytest.mark.parametrize("engine,n_src,n_tgt", [("auto", 1001, 1500), ("exact_f64", 300, 700)])
def test_no_pairs_ends_the_call(contexts, engine, n_src, n_tgt):
    c = contexts(engine)
    src, tgt = _room(n_src, n_tgt)
    far = src + np.array([100.0, 0.0, 0.0])
    (res, hist, pairs), small = _ran(c, lambda: c.align_gated(far, tgt, capi.Context.make_config(), 1.0))
    assert (small > 0) == (engine == "auto")
    assert hist.tolist() == [math.inf, math.inf] and res.final_error == math.inf
    assert not res.converged and res.num_iterations == 1 and res.loop_iterations == 1 and pairs == 0
    assert np.array_equal(_T(res), np.eye(4))
    # the post-loop pass alone (no iterations asked for) enters +Inf once
    res, hist, pairs = c.align_gated(far, tgt, capi.Context.make_config(max_iterations=0), 1.0)
    assert hist.tolist() == [math.inf] and res.num_iterations == 0 and not res.converged and pairs == 0
    # and the context goes on as before
    res, _hist, pairs = c.align_gated(src, tgt, capi.Context.make_config(), 5.0)
    assert res.converged and pairs == n_src


# ------------------------------------------------------------------------------------------------ batch, device pointers

def test_batch_is_the_sequential_calls_bit_for_bit(ctx, cases):
    s1, t1, start, _, _ = cases["l12_8_3"]
    s2, t2 = _room(1001, 4500)
    s3, t3 = _room(300, 700)
    srcs, tgts = [s1, s2, s3 + np.array([0.0, 100.0, 0.0])], [t1, t2, t3]
    cfgs = [capi.Context.make_config(30, 1e-6, initial_transform=start), capi.Context.make_config(), capi.Context.make_config(20)]
    gates = [GATE, 0.5, 1.0]
    alone = [ctx.align_gated(s, t, k, g) for s, t, k, g in zip(srcs, tgts, cfgs, gates)]
    together = ctx.align_gated_batch(srcs, tgts, cfgs, gates)
    for a, b in zip(alone, together):
        _same_bits(a, b)
        assert a[2] == b[2]
    assert together[2][2] == 0 and together[2][1].tolist() == [math.inf, math.inf]
    assert 0 < together[0][2] < s1.shape[0] and 0 < together[1][2] <= 1001


def test_device_pointers_give_the_host_call(ctx, cases):
    src, tgt, start, _, _ = cases["l12_6_5"]
    cfg = capi.Context.make_config(30, 1e-6, initial_transform=start)
    ds, dt_ = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    torch.cuda.synchronize()
    got = ctx.align_gated_device(ds.data_ptr(), src.shape[0], dt_.data_ptr(), tgt.shape[0], cfg, GATE)
    want = ctx.align_gated(src, tgt, cfg, GATE)
    _same_bits(got, want)
    assert got[2] == want[2]


# ------------------------------------------------------------------------------------------------ the detectors

def _key(r):
    return (r.query_frame, r.match_frame, r.sector_shift, r.pairs)


def _same_results(a, b):
    assert [_key(r) for r in a] == [_key(r) for r in b]
    for x, y in zip(a, b):
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


def _l12_cfg(gate):
    return lc.LoopClosureConfig(yaw_guess=True, max_correspondence_distance=gate, **ref.L12_CONFIG)


def test_l12_detectors_agree_and_match_the_restatement(tmp_path, ctx, oracle, l12):
    poses, labels, clouds = l12
    got = _host_and_store(ctx, clouds, labels, _l12_cfg(GATE))
    assert {r.query_frame for r in got} == set(range(100, 106))
    backend = ref.GatedOracleBackend(GATE, oracle)
    want = ref.run_detector(yr.YawLoopClosureDetector(backend, ref.l12_config()), clouds, labels)
    assert backend.min_margin() > 1e-9
    assert [_key(r) for r in got] == [(w.query_frame, w.match_frame, w.sector_shift, backend.run_of(w).pairs) for w in want]
    for a, b in zip(got, want):
        assert _bits([a.scan_context_distance]) == _bits([b.scan_context_distance])
        dt, dr = synth.pose_delta(np.asarray(a.transform), np.asarray(b.transform))
        assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD and abs(a.icp_fitness - b.icp_fitness) <= HIST_ATOL
    # without the gate some return scan stays open, and no result carries pairs
    off = _host_and_store(ctx, clouds, labels, _l12_cfg(0.0))
    assert set(range(100, 106)) - {r.query_frame for r in off} and all(r.pairs is None for r in off)

    # the C++ mirror (tests/cpp/gated_demo.cpp): both detectors and one align_gated, the same numbers
    from lidar_slam_from_scratch_amd import build
    exe = tmp_path / "gated_demo"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "gated_demo.cpp"), "-o", str(exe), build.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(build.LIB_PATH), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lamdhip64"])
    args = []
    for k, (c, label) in enumerate(zip(clouds, labels)):
        c.tofile(tmp_path / ("c%d.f64" % k))
        args += [str(label), str(tmp_path / ("c%d.f64" % k))]
    kw = ref.L12_CONFIG
    subprocess.check_call([str(exe), str(tmp_path / "o.f64"), str(kw["frame_gap"]), repr(kw["sc_distance_threshold"]),
                           repr(kw["icp_fitness_threshold"]), str(kw["max_candidates"]), "1", repr(GATE)] + args)
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
    res, _hist, pairs = ctx.align_gated(clouds[-1], clouds[0], capi.Context.make_config(30), GATE)
    assert (int(o[p]), int(o[p + 1]), int(o[p + 2]), int(o[p + 3])) == (pairs, clouds[-1].shape[0], res.converged, res.num_iterations)
    assert o[p + 4] == res.final_error and (o[p + 5:p + 21].reshape(4, 4) == _T(res)).all()
    assert p + 21 == o.size


def test_set_gate_zero_restores_the_ungated_results(ctx):
    poses, labels = yr.r12_reverse_drive()
    clouds = yr.scans(poses)
    cfg = dict(frame_gap=50, sc_distance_threshold=0.2, icp_fitness_threshold=0.3)   # tests/test_gpu_loop_yaw.py's R12

    def drive(switch_off_at):
        store = GlobalMap(ctx)
        det = lc.StoreLoopClosureDetector(ctx, store, lc.LoopClosureConfig(yaw_guess=True, **cfg))
        if switch_off_at is not None:
            det.set_gate(GATE)
        found = []
        for k, (cloud, label) in enumerate(zip(clouds, labels)):
            if k == switch_off_at:
                det.set_gate(0.0)
            store.add_frame(cloud)
            det.add_frame(store.size()[0] - 1, label)
            found.append(det.detect())
        det.close()
        store.close()
        return found

    plain, switched = drive(None), drive(9)
    assert sum(len(f) for f in plain) == 9                # what tests/test_gpu_loop_yaw.py finds on R12
    assert any(r.pairs is not None and r.pairs > 0 for f in switched[:9] for r in f)     # the gate was on ...
    for a, b in zip(plain[9:], switched[9:]):            # ... and off again: today's results, bit for bit
        assert len(a) > 0 and all(r.pairs is None for r in b)
        _same_results(a, b)
    lib = capi.load_library()
    store = GlobalMap(ctx)
    det = lc.StoreLoopClosureDetector(ctx, store)
    for bad in (-1.0, math.nan, math.inf):
        assert lib.icpmi_loop_set_gate(det._h, bad) == capi.ERR_ARG
    assert lib.icpmi_loop_set_gate(None, 1.0) == capi.ERR_NULL
    n = C.c_int64(-1)
    assert lib.icpmi_loop_last_pairs(det._h, None, 0, C.byref(n)) == capi.OK and n.value == 0
    det.close()
    store.close()


def test_run_slam_closes_a_return_leg_a_lane_aside(ctx):
    """D78 with the return leg 1.5 m aside and 3 degrees off the opposite heading.  DESIGN 7.8 records both errors; the
    assertion is the ordering alone."""
    poses = ref.d78l_lateral_drive()
    frames = yr.scans(poses)
    want = np.linalg.inv(poses[0]) @ poses[-1]
    on = slam.run_slam(frames, ctx, loop_yaw_guess=True, loop_gate=GATE)
    off = slam.run_slam(frames, ctx, loop_yaw_guess=True)
    e_on, e_off = synth.pose_delta(on.poses[-1], want), synth.pose_delta(off.poses[-1], want)
    print("D78L final pose error: gate", e_on, len(on.closures), "closures; no gate", e_off, len(off.closures), "closures")
    assert any(c.query_frame - c.match_frame >= 50 and c.pairs > 0 for c in on.closures)
    assert all(c.pairs is None for c in off.closures)
    assert off.closures == [] or e_on[0] <= e_off[0]


# ------------------------------------------------------------------------------------------------ error codes

def test_error_codes(ctx):
    lib = capi.load_library()
    src, tgt = _room(300, 700)
    cfg = capi.Context.make_config()
    for bad in (0.0, -2.0, math.nan, math.inf, -math.inf):
        with pytest.raises(capi.IcpError) as e:
            ctx.align_gated(src, tgt, cfg, bad)
        assert e.value.code == capi.ERR_ARG
        with pytest.raises(capi.IcpError) as e:
            ctx.align_gated_batch([src], [tgt], cfg, bad)
        assert e.value.code == capi.ERR_ARG
    hist, res = np.zeros(51), capi.Result()
    assert lib.icpmi_align_gated(ctx._h, capi._dp(src), 300, capi._dp(tgt), 700, C.byref(cfg), None, C.byref(res), None,
                                 capi._dp(hist), 51) == capi.ERR_NULL      # no gate: that is icpmi_align
    gate = capi.Gate()
    gate.max_distance = 1e6
    assert lib.icpmi_align_gated(ctx._h, capi._dp(src), 300, capi._dp(tgt), 700, C.byref(cfg), C.byref(gate), C.byref(res),
                                 None, capi._dp(hist), 51) == capi.OK      # info may be NULL
    assert lib.icpmi_align_gated(ctx._h, capi._dp(src), 300, capi._dp(tgt), 700, C.byref(cfg), C.byref(gate), C.byref(res),
                                 None, capi._dp(hist), 50) == capi.ERR_CAPACITY
    # a context with a communicator (the callbacks form, one rank) does not run gated registrations
    c = capi.Context(device=0)
    c.comm_init_callbacks(1, 0, lambda buf: None, lambda buf, per: None)
    with pytest.raises(capi.IcpError) as e:
        c.align_gated(src, tgt, cfg, 2.0)
    assert e.value.code == capi.ERR_ARG
    with pytest.raises(capi.IcpError) as e:
        c.align_gated_batch([src], [tgt], cfg, 2.0)
    assert e.value.code == capi.ERR_ARG
    c.comm_finalize()
    res, _hist, pairs = c.align_gated(src, tgt, cfg, 2.0)             # and does again without one
    assert res.converged and pairs > 0
    c.close()
