"""The loop-closure detector with its database on the device (icpmi_loop_*, csrc/loop_store.h,
loop_closure.StoreLoopClosureDetector) against today's host detector, LoopClosureDetector(GpuBackend(ctx)), fed the same
clouds, and against icpmi_scan_context: descriptors, candidates, distances, transforms and fitness bit for bit."""
import ctypes as C

import numpy as np
import pytest

import torch  # noqa: F401  (first: one HIP runtime per process)

from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402
from lidar_slam_from_scratch_amd import loop_closure as lc  # noqa: E402
from lidar_slam_from_scratch_amd import slam  # noqa: E402
from lidar_slam_from_scratch_amd.global_map import GlobalMap  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    """Fails loudly (no skip, no fallback) when the HIP library or the device is missing."""
    from lidar_slam_from_scratch_amd import build
    build.build_library()
    c = capi.Context(device=0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_results(a, b):
    assert [(r.query_frame, r.match_frame) for r in a] == [(r.query_frame, r.match_frame) for r in b]
    for x, y in zip(a, b):
        assert _bits([x.scan_context_distance]) == _bits([y.scan_context_distance])
        assert _bits([x.icp_fitness]) == _bits([y.icp_fitness])
        assert np.array_equal(_bits(x.transform), _bits(y.transform))


def _off_sector_boundaries(cloud):
    """(as tests/test_gpu_parity.py) points whose azimuth is not within 1e-9 of a Scan Context sector boundary"""
    q = (np.arctan2(cloud[:, 1], cloud[:, 0]) + np.pi) / (2 * np.pi / 60)
    return cloud[np.abs(q - np.round(q)) > 1e-9]


class Pair:
    """The host detector and the store detector, fed the same frames; the store may hold other frames between them."""

    def __init__(self, ctx, cfg, store=None):
        self.store = store if store is not None else GlobalMap(ctx)
        self.host = lc.LoopClosureDetector(lc.GpuBackend(ctx), cfg)
        self.dev = lc.StoreLoopClosureDetector(ctx, self.store, cfg)

    def add(self, cloud, label, filler=None):
        if filler is not None:                      # a store frame no entry names (a too-few-points frame)
            self.store.add_frame(filler)
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


def _drive(frames, **kw):
    return [synth.lidar_frame(f, beams=32, azimuths=900, **kw) for f in frames]


# ---------------------------------------------------------------------------------------------------------------- descriptors

def test_descriptors_bit_exact(ctx):
    rng = np.random.default_rng(7)
    lidar = _drive([0, 5, 11])
    nan_rows = lidar[0].copy()
    nan_rows[::17, 2] = np.nan
    nan_rows[5::23, 0] = np.nan
    nan_rows[9::31, 1] = np.nan
    edge = np.array([[0.1, 0.0, 1.0], [0.0, 0.1, 2.0], [80.0, 0.0, 3.0], [0.0, -80.0, 4.0], [np.nextafter(0.1, 0), 0, 5.0],
                     [np.nextafter(80.0, 100), 0, 6.0], [-80.0, 1e-300, 7.0], [56.568542494923804, 56.568542494923804, 8.0]])
    big = np.c_[rng.uniform(-90, 90, (130000, 2)), rng.uniform(-3, 20, 130000)]
    one = np.array([[3.0, 4.0, 1.5]])
    frames = [one, lidar[0], np.zeros((0, 3)), nan_rows, edge, big, lidar[1], lidar[2]]
    store = GlobalMap(ctx)
    det = lc.StoreLoopClosureDetector(ctx, store)
    # one at a time: each entry is described on its own (the first frame of 1 row puts every later frame at an odd row
    # offset, 8-byte aligned only)
    for i, f in enumerate(frames[:4]):
        store.add_frame(f)
        det.add_frame(i, i)
        assert np.array_equal(_bits(det.descriptor(i)), _bits(ctx.scan_context(f))), i
    # in one batch: four pending entries, described by the first call that needs them
    for i, f in enumerate(frames[4:], start=4):
        store.add_frame(f)
        det.add_frame(i, i)
    assert store.size()[1] % 2 == 1
    for i in range(len(frames) - 1, -1, -1):
        assert np.array_equal(_bits(det.descriptor(i)), _bits(ctx.scan_context(frames[i]))), i
    assert not det.descriptor(2).any()                     # 0 rows: every bin empty
    det.close()
    store.close()


# ---------------------------------------------------------------------------------------------------------------- detect parity

def test_detect_parity_revisit_drive(ctx):
    """test_gpu_parity.py::test_loop_closure_detector_matches_oracle's drive: frames 1 and 3 revisit the start"""
    order = [0, 2, 4, 6, 8, 10, 12, 1, 3]
    clouds = [_off_sector_boundaries(c) for c in _drive(order)]
    cfg = lc.LoopClosureConfig(frame_gap=5, sc_distance_threshold=0.2, icp_fitness_threshold=0.3)
    p = Pair(ctx, cfg)
    found = []
    for k, c in enumerate(clouds):
        p.add(c, k)
        found += p.detect()
    assert len(found) >= 1
    p.close()


def test_detect_parity_out_and_back(ctx):
    """test_gpu_pose_graph.py::test_run_slam_out_and_back's street, 60 frames out and 60 back, a detect after every add"""
    order = list(range(60)) + list(range(59, -1, -1))
    cache = dict(zip(range(60), _drive(range(60), **synth.DRIVE_200)))
    p = Pair(ctx, slam.node_loop_config())
    found = []
    for k, f in enumerate(order):
        p.add(cache[f], k)
        found += p.detect()
    assert any(r.query_frame - r.match_frame >= 50 for r in found)
    p.close()


# ---------------------------------------------------------------------------------------------------------------- candidate rules

def test_label_gap_edges_and_non_increasing_labels(ctx):
    c = _drive([3])[0]
    cfg = lc.LoopClosureConfig(frame_gap=5, sc_distance_threshold=0.25, icp_fitness_threshold=0.3, max_candidates=3)
    p = Pair(ctx, cfg)
    p.add(c, 10)
    p.add(c, 11)
    p.add(c, 15)                                   # gap 5 to label 10: in; gap 4 to label 11: out
    assert [r.match_frame for r in p.detect()] == [10]
    for label in (3, 40, 2, 9, 0, 30):             # labels need not increase
        p.add(c, label)
        p.detect()
    p.close()


def test_distance_exactly_at_threshold_is_excluded(ctx):
    a, b = [synth.lidar_frame(20, beams=32, azimuths=900, range_noise=s) for s in (0.01, 0.02)]   # one place, two noises
    d = ctx.scan_context_distances(ctx.scan_context(b), ctx.scan_context(a)[None])[0]
    assert 0 < d < 1
    for thr, n in ((d, 0), (np.nextafter(d, 2.0), 1)):
        cfg = lc.LoopClosureConfig(frame_gap=1, sc_distance_threshold=float(thr), icp_fitness_threshold=10.0)
        p = Pair(ctx, cfg)
        p.add(a, 0)
        p.add(b, 1)
        assert len(p.detect()) == n
        p.close()


def test_equal_distances_order_by_entry(ctx):
    """one store frame named by two entries: equal distances, the lower entry first"""
    a, q = [synth.lidar_frame(30, beams=32, azimuths=900, range_noise=s) for s in (0.01, 0.02)]
    cfg = lc.LoopClosureConfig(frame_gap=1, sc_distance_threshold=0.5, icp_fitness_threshold=10.0, max_candidates=1)
    p = Pair(ctx, cfg)
    p.add(a, 7)
    p.host.add_frame(a, 4)                           # the same cloud again, the same store frame
    p.dev.add_frame(p.store.size()[0] - 1, 4)
    p.add(q, 20)
    r = p.detect()
    assert [x.match_frame for x in r] == [7]
    p.close()


@pytest.mark.parametrize("max_candidates", [0, 1, 3, 10])
def test_max_candidates(ctx, max_candidates):
    """one place at twelve noise levels: more candidates than ICPMI_MAX_BATCH, so 10 takes two rounds"""
    clouds = [synth.lidar_frame(40, beams=32, azimuths=900, range_noise=0.01 + 0.002 * s) for s in range(12)]
    cfg = lc.LoopClosureConfig(frame_gap=1, sc_distance_threshold=0.6, icp_fitness_threshold=10.0,
                               max_candidates=max_candidates)
    p = Pair(ctx, cfg)
    for k, c in enumerate(clouds):
        p.add(c, k)
    r = p.detect()
    assert len(r) == min(max_candidates, 11)
    p.close()


def _bin_skeleton(cloud):
    """per Scan Context bin the highest point only: the same descriptor, a much worse registration target"""
    rng_ = np.sqrt(cloud[:, 0] ** 2 + cloud[:, 1] ** 2)
    ang = np.arctan2(cloud[:, 1], cloud[:, 0]) + np.pi
    ok = (rng_ <= 80.0) & (rng_ >= 0.1)
    ring = np.clip((rng_ / 4.0).astype(int), 0, 19)
    sector = np.clip((ang / (2 * np.pi / 60)).astype(int), 0, 59)
    key = np.where(ok, ring * 60 + sector, -1)
    keep = []
    for k in np.unique(key[key >= 0]):
        idx = np.nonzero(key == k)[0]
        keep.append(idx[np.argmax(cloud[idx, 2])])
    return cloud[np.sort(keep)]


def test_rejected_first_candidates_then_later_ones(ctx):
    c = _off_sector_boundaries(_drive([50])[0])
    sk = _bin_skeleton(c)
    assert np.array_equal(ctx.scan_context(sk), ctx.scan_context(c))
    loose = lc.LoopClosureConfig(frame_gap=1, sc_distance_threshold=0.5, icp_fitness_threshold=1e300, max_candidates=10)
    p = Pair(ctx, loose)
    for label, cloud in ((0, sk), (1, sk), (2, c), (9, c)):
        p.add(cloud, label)
    every = p.detect()                             # equal distances: entries 0, 1 (skeletons), 2 verified in that order
    p.close()
    got = [r.match_frame for r in every]
    assert got[-1] == 2 and set(got) <= {0, 1, 2}
    fit = {r.match_frame: r.icp_fitness for r in every}
    # the skeletons either fail to converge (rejected at any threshold) or register worse than the cloud itself
    thr = min([fit[e] for e in (0, 1) if e in fit] + [0.3])
    assert fit[2] < thr
    strict = lc.LoopClosureConfig(frame_gap=1, sc_distance_threshold=0.5, icp_fitness_threshold=thr, max_candidates=1)
    p = Pair(ctx, strict)
    for label, cloud in ((0, sk), (1, sk), (2, c), (9, c)):
        p.add(cloud, label)
    assert [r.match_frame for r in p.detect()] == [2]   # entries 0 and 1 verified and rejected, then entry 2
    p.close()


def test_entries_skip_store_frames(ctx):
    order = [0, 2, 4, 6, 8, 10, 12, 1, 3]
    clouds = [_off_sector_boundaries(c) for c in _drive(order)]
    cfg = lc.LoopClosureConfig(frame_gap=5, sc_distance_threshold=0.2, icp_fitness_threshold=0.3)
    p = Pair(ctx, cfg)
    few = clouds[0][:7]
    for k, c in enumerate(clouds):
        p.add(c, 2 * k, filler=few if k % 2 else None)
        p.detect()
    assert p.store.size()[0] == len(clouds) + len(clouds) // 2 and p.dev.size() == len(clouds)
    p.close()


# ---------------------------------------------------------------------------------------------------------------- store growth

def test_store_growth_between_adds_and_detect(ctx):
    order = [0, 2, 4, 6, 8, 10, 12, 1, 3]
    clouds = [_off_sector_boundaries(c) for c in _drive(order)]
    cfg = lc.LoopClosureConfig(frame_gap=5, sc_distance_threshold=0.2, icp_fitness_threshold=0.3)
    rng = np.random.default_rng(3)
    p = Pair(ctx, cfg)
    found = []
    for k, c in enumerate(clouds):
        p.add(c, k)
        if k % 3 == 1:                              # grow the arena (and move it) before the pending entries are described
            p.store.add_frame(rng.uniform(-50, 50, (200000 * (k + 1), 3)))
        found += p.detect()
        for e in range(p.dev.size()):
            assert np.array_equal(_bits(p.dev.descriptor(e)), _bits(p.host._descriptors[e].reshape(20, 60)))
    assert found
    p.close()


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


def test_run_slam_loop_on_device(ctx):
    order = list(range(60)) + list(range(59, -1, -1))
    cache = dict(zip(range(60), _drive(range(60), **synth.DRIVE_200)))
    frames = [cache[f] for f in order]
    base = slam.run_slam(frames, ctx)
    assert base.closures
    _same_run(base, slam.run_slam(frames, ctx, loop_on_device=True))
    gm = GlobalMap(ctx)
    for f in frames[:3]:                            # a caller's map that already holds frames: store index != k
        gm.add_frame(f)
    run = slam.run_slam(frames, ctx, global_map=gm, loop_on_device=True)
    _same_run(base, run)
    assert gm.size()[0] == 3 + len(frames)
    gm.close()
    with pytest.raises(ValueError):
        slam.run_slam(frames[:2], ctx, loop_backend=lc.GpuBackend(ctx), loop_on_device=True)


# ---------------------------------------------------------------------------------------------------------------- errors, lifetime

def test_error_paths_and_destroy_order(ctx):
    lib = capi.load_library()
    a, b = [synth.lidar_frame(0, beams=32, azimuths=900, range_noise=s) for s in (0.01, 0.02)]
    store = GlobalMap(ctx)
    store.add_frame(a)
    det = lc.StoreLoopClosureDetector(ctx, store, lc.LoopClosureConfig(frame_gap=1, sc_distance_threshold=0.9,
                                                                      icp_fitness_threshold=10.0))
    assert det.detect() == []                                      # no entries
    for bad in (-1, 1, 5):
        with pytest.raises(capi.IcpError) as e:
            det.add_frame(bad, 0)
        assert e.value.code == capi.ERR_ARG and det.size() == 0
    det.add_frame(0, 0)
    assert det.detect() == []                                      # one entry
    for bad in (-1, 1):
        with pytest.raises(capi.IcpError) as e:
            det.descriptor(bad)
        assert e.value.code == capi.ERR_ARG
    store.add_frame(b)
    det.add_frame(1, 1)
    n = C.c_int64(0)
    assert lib.icpmi_loop_detect(det._h, None, 0, C.byref(n)) == capi.ERR_CAPACITY and n.value == 1
    assert len(det.detect()) == 1
    det.clear()
    assert det.size() == 0 and store.size()[0] == 2 and det.detect() == []
    det.add_frame(1, 0)
    det.add_frame(0, 5)
    assert [r.match_frame for r in det.detect()] == [0]
    # an empty store frame as a candidate: the verification's error, as icpmi_align_batch returns it
    store.add_frame(np.zeros((0, 3)))
    cfg1 = lc.LoopClosureConfig(frame_gap=1, sc_distance_threshold=1.5, icp_fitness_threshold=10.0)
    d2 = lc.StoreLoopClosureDetector(ctx, store, cfg1)
    d2.add_frame(2, 0)
    d2.add_frame(1, 9)
    with pytest.raises(capi.IcpError) as e:
        d2.detect()
    assert e.value.code == capi.ERR_EMPTY_TARGET
    # a context with a communicator is refused at detect
    c2 = capi.Context(device=0)
    c2.comm_init_callbacks(1, 0, lambda arr: None, lambda arr, per: None)
    s2 = GlobalMap(c2)
    s2.add_frame(a)
    s2.add_frame(b)
    d3 = lc.StoreLoopClosureDetector(c2, s2)
    d3.add_frame(0, 0)
    d3.add_frame(1, 100)
    with pytest.raises(capi.IcpError) as e:
        d3.detect()
    assert e.value.code == capi.ERR_ARG
    c2.close()                                                      # closes d3, then s2, then the context
    assert d3._h is None and s2._h is None
    # destroy order by hand: the detector, its map, (the context at the fixture's end)
    d2.close()
    det.close()
    det.close()
    store.close()
