"""Loop closures on revisits with another heading on the device: k_sc_distances_shift and
k_loop_candidates_shift against the CPU restatement (scripts/loop_yaw_ref.py), the three detectors with yaw_guess
against each other bit for bit and against the restatement's detector on the oracle, icpmi_loop_last_shifts, the node's
loop through slam.run_slam, and the C++ mirror (tests/cpp/loop_yaw_demo.cpp).  The drives are loop_yaw_ref's: R12 (a
street driven back facing the other way), H12 (one place, twelve headings), D78 (out, turn round, back) and the
existing revisit drive V9, where every shift is 0."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import torch  # noqa: F401  (first: one HIP runtime per process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import loop_yaw_ref as ref  # noqa: E402
from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402
from lidar_slam_from_scratch_amd import loop_closure as lc  # noqa: E402
from lidar_slam_from_scratch_amd import slam  # noqa: E402
from lidar_slam_from_scratch_amd.global_map import GlobalMap  # noqa: E402

pytestmark = pytest.mark.gpu

POSE_TOL_M, POSE_TOL_RAD = 1e-4, 1e-4   # tests/test_gpu_parity.py's north_star tolerance
R12_CFG = dict(frame_gap=50, sc_distance_threshold=0.2, icp_fitness_threshold=0.3)
H12_CFG = dict(frame_gap=1, sc_distance_threshold=0.25, icp_fitness_threshold=0.3, max_candidates=10)


@pytest.fixture(scope="module")
def ctx():
    """Fails loudly (no skip, no fallback) when the HIP library or the device is missing."""
    from lidar_slam_from_scratch_amd import build
    build.build_library()
    c = capi.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def r12():
    poses, labels = ref.r12_reverse_drive()
    return poses, labels, ref.scans(poses)


@pytest.fixture(scope="module")
def h12():
    poses, labels = ref.h12_headings()
    return poses, labels, ref.scans(poses)


@pytest.fixture(scope="module")
def v9():
    order = [0, 2, 4, 6, 8, 10, 12, 1, 3]          # frames 1 and 3 revisit the start of the drive, facing the same way
    return [ref.off_sector_boundaries(synth.lidar_frame(f, beams=32, azimuths=900)) for f in order]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_results(a, b):
    assert [(r.query_frame, r.match_frame, r.sector_shift) for r in a] == [(r.query_frame, r.match_frame, r.sector_shift) for r in b]
    for x, y in zip(a, b):
        assert _bits([x.scan_context_distance]) == _bits([y.scan_context_distance])
        assert _bits([x.icp_fitness]) == _bits([y.icp_fitness])
        assert np.array_equal(_bits(x.transform), _bits(y.transform))


class Pair:
    """tests/test_gpu_loop_store.py's idiom: the host detector and the store detector, fed the same frames.  A store
    frame of one row goes first, so that every entry sits at an odd row offset (8-byte aligned only)."""

    def __init__(self, ctx, cfg):
        self.store = GlobalMap(ctx)
        self.store.add_frame(np.array([[3.0, 4.0, 1.5]]))
        self.host = lc.LoopClosureDetector(lc.GpuBackend(ctx), cfg)
        self.dev = lc.StoreLoopClosureDetector(ctx, self.store, cfg)

    def add(self, cloud, label):
        self.store.add_frame(cloud)
        self.host.add_frame(cloud, label)
        self.dev.add_frame(self.store.size()[0] - 1, label)

    def detect(self):
        a, b = self.host.detect(), self.dev.detect()
        _same_results(a, b)
        return b

    def close(self):
        self.dev.close()
        self.store.close()


def _pair_drive(ctx, clouds, labels, cfg, every=True):
    p = Pair(ctx, cfg)
    found = []
    for k, (c, label) in enumerate(zip(clouds, labels)):
        p.add(c, label)
        if every or k == len(clouds) - 1:
            found += p.detect()
    p.close()
    return found


def _oracle_drive(oracle, clouds, labels, cfg, every=True):
    det = ref.YawLoopClosureDetector(ref.OracleBackend(oracle), cfg)
    found = []
    for k, (c, label) in enumerate(zip(clouds, labels)):
        det.add_frame(c, label)
        if every or k == len(clouds) - 1:
            found += det.detect()
    return found


def _against_oracle(got, want):
    assert [(r.query_frame, r.match_frame, r.sector_shift) for r in got] == [(r.query_frame, r.match_frame, r.sector_shift) for r in want]
    for a, b in zip(got, want):
        assert _bits([a.scan_context_distance]) == _bits([b.scan_context_distance])
        dt, dr = synth.pose_delta(np.asarray(a.transform), np.asarray(b.transform))
        print("  (%d, %d) shift %d: %.3e m %.3e rad, fitness differs by %.3e"
              % (a.query_frame, a.match_frame, a.sector_shift, dt, dr, abs(a.icp_fitness - b.icp_fitness)))
        assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD and abs(a.icp_fitness - b.icp_fitness) < 1e-9


# ---------------------------------------------------------------------------------------------------------------- the kernel

def _check_distances_shift(ctx, query, hist):
    hist = np.ascontiguousarray(hist)
    dist, shift = ctx.scan_context_distances_shift(query, hist)
    assert shift.dtype == np.int32 and dist.shape == shift.shape == (hist.shape[0],)
    assert np.array_equal(_bits(dist), _bits(ctx.scan_context_distances(query, hist)))
    want = [ref.distance_shift(query, h) for h in hist]
    assert shift.tolist() == [w[1] for w in want]
    assert np.array_equal(_bits(dist), _bits([w[0] for w in want]))
    return dist, shift


def test_distances_shift_rolls_zero_and_self(ctx, r12):
    D = ctx.scan_context(r12[2][0])
    hist = np.stack([np.roll(D, -s, axis=1) for s in range(60)] + [np.zeros((20, 60)), D])
    for count in (1, 2, 62):
        dist, shift = _check_distances_shift(ctx, D, hist[:count])
    assert shift[:60].tolist() == [(-s) % 60 for s in range(60)] and shift[61] == 0
    assert (dist[60], shift[60]) == (1.0, 0)                     # zero-norm descriptor: 1 at every shift, the first stays
    for s in (1, 17, 59):                                         # the query rolled: the shift is the roll itself
        assert ctx.scan_context_distances_shift(np.roll(D, -s, axis=1), D[None])[1].tolist() == [s]
    assert ctx.scan_context_distances_shift(D, np.zeros((0, 20, 60)))[0].shape == (0,)


def test_distances_shift_ties_go_to_the_smaller_shift(ctx):
    half = np.random.default_rng(5).integers(0, 8, (20, 30)).astype(np.float64)
    P = np.concatenate([half, half], axis=1)                      # period 30 sectors, every sum exact
    hist = np.stack([np.roll(P, -s, axis=1) for s in range(60)])
    _, shift = _check_distances_shift(ctx, P, hist)
    assert shift.tolist() == [(-s) % 30 for s in range(60)]
    for s in (0, 7, 29, 30, 31, 59):
        assert ctx.scan_context_distances_shift(np.roll(P, -s, axis=1), P[None])[1].tolist() == [s % 30]


def test_distances_shift_on_real_descriptors(ctx, r12):
    descs = [ctx.scan_context(c) for c in r12[2]]
    for q in descs[6:]:
        _check_distances_shift(ctx, q, np.stack(descs[:6]))


# ---------------------------------------------------------------------------------------------------------------- the detectors

def test_r12_three_detectors(ctx, oracle, r12):
    poses, labels, clouds = r12
    cfg = lc.LoopClosureConfig(yaw_guess=True, **R12_CFG)
    on = _pair_drive(ctx, clouds, labels, cfg)
    first = {}
    for r in on:
        first.setdefault(r.query_frame, r)
    assert [(q, first[q].match_frame, first[q].sector_shift) for q in range(100, 106)] == \
        [(100, 5, 28), (101, 4, 28), (102, 3, 29), (103, 2, 29), (104, 1, 30), (105, 0, 30)]
    _against_oracle(on, _oracle_drive(oracle, clouds, labels, cfg))
    off = _pair_drive(ctx, clouds, labels, lc.LoopClosureConfig(**R12_CFG))
    assert off == []                                              # from the identity the return leg closes nothing


def test_h12_three_detectors(ctx, oracle, h12):
    poses, labels, clouds = h12
    cfg = lc.LoopClosureConfig(yaw_guess=True, **H12_CFG)
    on = _pair_drive(ctx, clouds, labels, cfg, every=False)      # ten verifications: two rounds, each problem its own start
    assert len(on) == 10 and len({r.sector_shift for r in on}) == 10
    _against_oracle(on, _oracle_drive(oracle, clouds, labels, cfg, every=False))
    off = _pair_drive(ctx, clouds, labels, lc.LoopClosureConfig(**H12_CFG), every=False)
    assert len(off) < 10 and all(r.sector_shift is None for r in off)


def test_v9_same_heading_changes_nothing(ctx, v9):
    kw = dict(frame_gap=5, sc_distance_threshold=0.2, icp_fitness_threshold=0.3)
    labels = list(range(len(v9)))
    off = _pair_drive(ctx, v9, labels, lc.LoopClosureConfig(**kw))
    on = _pair_drive(ctx, v9, labels, lc.LoopClosureConfig(yaw_guess=True, **kw))
    assert len(off) >= 1 and [r.sector_shift for r in on] == [0] * len(on)
    for r in on:
        r.sector_shift = None
    _same_results(on, off)


def test_last_shifts_and_toggle(ctx, r12, v9):
    lib = capi.load_library()
    _, labels, clouds = r12
    store = GlobalMap(ctx)
    det = lc.StoreLoopClosureDetector(ctx, store, lc.LoopClosureConfig(**R12_CFG))
    for k in (0, 1, 11):                                          # labels 0, 1 and 105: the last faces the other way
        store.add_frame(clouds[k])
        det.add_frame(store.size()[0] - 1, labels[k])
    n = C.c_int64(-1)
    buf = (C.c_int32 * 4)(7, 7, 7, 7)
    assert lib.icpmi_loop_last_shifts(det._h, buf, 4, C.byref(n)) == capi.OK and n.value == 0   # no detect yet
    assert det.detect() == []                                     # off
    assert lib.icpmi_loop_last_shifts(det._h, buf, 4, C.byref(n)) == capi.OK and n.value == 0
    before = [det.descriptor(e) for e in range(3)]
    raw = (capi.LoopResult * 3)()
    m = C.c_int64(0)
    ctx._check(lib.icpmi_loop_set_yaw_guess(det._h, 1))           # on: takes effect at the next detect
    ctx._check(lib.icpmi_loop_detect(det._h, raw, 3, C.byref(m)))
    assert [(raw[i].query_frame, raw[i].match_frame) for i in range(m.value)] == [(105, 0), (105, 1)]
    assert lib.icpmi_loop_last_shifts(det._h, buf, 4, C.byref(n)) == capi.OK and n.value == 2
    assert list(buf) == [30, 30, 7, 7]
    assert lib.icpmi_loop_last_shifts(det._h, buf, 1, C.byref(n)) == capi.ERR_CAPACITY and n.value == 2
    assert lib.icpmi_loop_last_shifts(det._h, None, 0, C.byref(n)) == capi.ERR_CAPACITY and n.value == 2
    assert lib.icpmi_loop_last_shifts(det._h, buf, 4, None) == capi.ERR_NULL
    for e in range(3):
        assert np.array_equal(_bits(det.descriptor(e)), _bits(before[e]))
    ctx._check(lib.icpmi_loop_set_yaw_guess(det._h, 0))          # off again: nothing closes, no shifts
    ctx._check(lib.icpmi_loop_detect(det._h, raw, 3, C.byref(m)))
    assert m.value == 0 and lib.icpmi_loop_last_shifts(det._h, buf, 4, C.byref(n)) == capi.OK and n.value == 0
    det.close()
    store.close()
    # with the guess off and results: one -1 per result
    store = GlobalMap(ctx)
    det = lc.StoreLoopClosureDetector(ctx, store, lc.LoopClosureConfig(frame_gap=5, sc_distance_threshold=0.2,
                                                                       icp_fitness_threshold=0.3))
    total = 0
    for k, c in enumerate(v9):
        store.add_frame(c)
        det.add_frame(k, k)
        if k >= len(v9) - 2:
            got = det.detect()
            assert all(r.sector_shift is None for r in got)
            assert lib.icpmi_loop_last_shifts(det._h, buf, 4, C.byref(n)) == capi.OK and n.value == len(got)
            assert list(buf)[:n.value] == [-1] * n.value
            total += len(got)
    assert total >= 1
    det.close()
    store.close()


# ---------------------------------------------------------------------------------------------------------------- run_slam

def _same_run(a, b):
    assert len(a.factors) == len(b.factors)
    for f, g in zip(a.factors, b.factors):
        assert f[0] == g[0] and len(f) == len(g)
        for x, y in zip(f[1:], g[1:]):
            if isinstance(x, np.ndarray):
                assert np.array_equal(_bits(x), _bits(y))
            else:
                assert x == y
    _same_results(a.closures, b.closures)
    assert [o[0] for o in a.optimizations] == [o[0] for o in b.optimizations]
    assert [o[1] for o in a.optimizations] == [o[1] for o in b.optimizations]
    assert np.array_equal(_bits(np.stack(a.poses)), _bits(np.stack(b.poses)))


def test_d78_run_slam(ctx):
    poses = ref.d78_drive()
    frames = ref.scans(poses)
    want = np.linalg.inv(poses[0]) @ poses[-1]
    off = slam.run_slam(frames, ctx)
    assert off.closures == []
    on = slam.run_slam(frames, ctx, loop_yaw_guess=True)
    assert any(c.query_frame == 70 and c.query_frame - c.match_frame >= 50 for c in on.closures)
    _same_run(on, slam.run_slam(frames, ctx, loop_yaw_guess=True, loop_on_device=True))
    e_off, e_on = synth.pose_delta(off.poses[-1], want), synth.pose_delta(on.poses[-1], want)
    print("D78 final pose error: off", e_off, "on", e_on, "closures", [(c.query_frame, c.match_frame, c.sector_shift) for c in on.closures])
    assert e_on[0] <= 0.5 * e_off[0] and e_on[1] <= 0.5 * e_off[1]


# ---------------------------------------------------------------------------------------------------------------- C++ mirror

def test_cpp_loop_yaw_mirror(tmp_path, ctx, r12):
    """include/icp_mi355x.hpp's two detectors with yaw_guess from a plain C++17 program against the Python mirror
    through the same C ABI: the same closures and shifts, the same bits"""
    from lidar_slam_from_scratch_amd import build
    exe = tmp_path / "loop_yaw_demo"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "loop_yaw_demo.cpp"), "-o", str(exe), build.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(build.LIB_PATH), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lamdhip64"])
    _, labels, clouds = r12
    args = []
    for k, (c, label) in enumerate(zip(clouds, labels)):
        c.tofile(tmp_path / ("c%d.f64" % k))
        args += [str(label), str(tmp_path / ("c%d.f64" % k))]
    text = subprocess.check_output([str(exe), str(tmp_path / "o.f64"), "50", "0.2", "0.3", "3", "1"] + args, text=True)
    assert "shift 28" in text and "shift 30" in text
    o = np.fromfile(tmp_path / "o.f64")
    det = lc.LoopClosureDetector(lc.GpuBackend(ctx), lc.LoopClosureConfig(yaw_guess=True, **R12_CFG))
    want = []
    for c, label in zip(clouds, labels):
        det.add_frame(c, label)
        want.extend(det.detect())
    assert len(want) == 9
    p = 0
    for _detector in ("host", "store"):
        assert int(o[p]) == len(want)
        p += 1
        for w in want:
            assert (int(o[p]), int(o[p + 1]), int(o[p + 2])) == (w.query_frame, w.match_frame, w.sector_shift)
            assert o[p + 3] == w.scan_context_distance and o[p + 4] == w.icp_fitness
            assert (o[p + 5:p + 21].reshape(4, 4) == np.asarray(w.transform).reshape(4, 4)).all()
            p += 21
    assert p == o.size
