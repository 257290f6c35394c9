"""The later trips of four loops, on the device (the inputs and their restatements: tests/loop_trip_inputs.py, held to
their preconditions by tests/test_loop_trip_inputs.py):

    k_voxel_centroids   a voxel of more than 64 rows: the serial sums carry on from one 64-row chunk into the next
    k_bbox_partial      the voxel filter's box over more than 256 x 256 rows
    k_lmap_keys, k_lmap_marks, k_lmap_merge   more than kLmapMaxBlocks x 256 scan rows / table elements
    k_transform         more than 2048 x 256 rows (the second row of a thread's batch), more than kRowBatch times that (the
                        second trip of its loop); the registration loop's movers past that size

Everything but the registration is compared byte for byte -- with the oracle's filter (oracle/icp_oracle.c), a Python
loop that adds a voxel's rows in input order, the local map's restatement (scripts/local_map_ref.py), the unfused
row-by-row product; the registration within tests/test_gpu_parity.py's check_against."""
import os
import sys

import numpy as np
import pytest

import torch  # noqa: F401  (first: one HIP runtime per process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import local_map_ref as lm  # noqa: E402
import loop_trip_inputs as inputs  # noqa: E402
from lidar_slam_from_scratch_amd import capi, synth  # noqa: E402
from lidar_slam_from_scratch_amd.local_map import LocalMap, LocalMapConfig  # noqa: E402
from test_gpu_local_map import add_both, same_table  # noqa: E402
from test_gpu_parity import check_against  # noqa: E402

pytestmark = pytest.mark.gpu

I4 = np.eye(4)
VOXEL = inputs.VOXEL


@pytest.fixture(scope="module")
def ctx():
    """Fails loudly (no skip, no fallback) when the HIP library or the device is missing."""
    from lidar_slam_from_scratch_amd import build
    build.build_library()
    c = capi.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def default_frame():
    """the default 64 x 1800 raw frame: made once, shared, left unchanged"""
    raw = synth.lidar_frame(0, voxel=None)
    assert raw.shape == (114606, 3) and raw.shape[0] > inputs.BBOX_ROWS
    raw.setflags(write=False)
    return raw


def same_bytes(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    assert got.tobytes() == want.tobytes()


def filter_on_device(ctx, cloud, voxel):
    """icpmi_voxel_downsample_device on torch memory -> the centroids back on the host"""
    d_in = torch.from_numpy(np.array(cloud, dtype=np.float64)).cuda()
    d_out = torch.full_like(d_in, 7.0)
    torch.cuda.synchronize()                                     # (torch's copies run on another stream than the context's)
    n = ctx.voxel_downsample_device(d_in.data_ptr(), d_in.shape[0], voxel, d_out.data_ptr(), d_out.shape[0])
    return d_out[:n].cpu().numpy()


# ------------------------------------------------------------------ 1. dense voxels
@pytest.mark.parametrize("reverse", [False, True], ids=["as_made", "reversed"])
def test_dense_voxels_sum_in_input_order(ctx, oracle, reverse):
    """voxels of 1 .. 5,000 rows, run lengths on both sides of every multiple of 64 up to 192, rows scattered through the
    input: host form and device form are the oracle's bytes, and those are the sequential sum's.  Reversing the input
    changes the sums (tests/test_loop_trip_inputs.py); parity must hold all the same."""
    cloud, _ = inputs.dense_cloud()
    if reverse:
        cloud = np.ascontiguousarray(cloud[::-1])
    want = oracle.voxel_downsample(cloud, VOXEL)
    loop, counts = inputs.centroids_by_loop(cloud, VOXEL)
    assert sorted(counts) == sorted(inputs.RUNS)
    same_bytes(want, loop)
    same_bytes(ctx.voxel_downsample(cloud, VOXEL), want)
    same_bytes(filter_on_device(ctx, cloud, VOXEL), want)


def test_default_frame_host_and_device_forms(ctx, oracle, default_frame):
    """114,606 rows: voxels of up to 223 rows next to the sensor, and k_bbox_partial past its 65,536 rows"""
    want = oracle.voxel_downsample(default_frame, VOXEL)
    assert 5000 < want.shape[0] < default_frame.shape[0]
    same_bytes(ctx.voxel_downsample(default_frame, VOXEL), want)
    same_bytes(filter_on_device(ctx, default_frame, VOXEL), want)


def test_default_frame_through_the_file_routes(tmp_path, oracle, default_frame):
    """The frame as float32 records (whose sums are exact in any order: this is about the chunks, not the order).  A plain
    icpmi_stream_push_file filters on the context's stream with the run count read back first.  Behind
    icpmi_stream_prefetch_file the worker queues the whole filter -- k_voxel_centroids launched for every row and reading
    the run count from the device -- once a push has told it the voxel size: hence the first pair of calls."""
    rec = inputs.as_bin_records(default_frame)
    paths = [str(tmp_path / ("%06d.bin" % k)) for k in range(3)]
    for p in paths:
        rec.tofile(p)
    want = oracle.voxel_downsample(capi.load_cloud(paths[0]), VOXEL)
    assert 5000 < want.shape[0] < rec.shape[0]
    cfg = capi.Context.make_config()
    c = capi.Context(device=0)
    _res, _hist, info = c.stream_push_file(paths[0], VOXEL, 1000, cfg)
    assert info.status == capi.STREAM_FIRST_FRAME and info.n_filtered == want.shape[0]
    same_bytes(c.stream_current_scan(), want)
    c.stream_reset()
    c.stream_prefetch_file(paths[1])                            # (no voxel size yet: the worker only uploads and widens)
    _res, _hist, info = c.stream_push_file(paths[1], VOXEL, 1000, cfg)
    assert info.status == capi.STREAM_FIRST_FRAME and info.n_filtered == want.shape[0]
    same_bytes(c.stream_current_scan(), want)
    c.stream_prefetch_file(paths[2])                            # the deferred filter
    res, _hist, info = c.stream_push_file(paths[2], VOXEL, 1000, cfg)
    assert info.status == capi.STREAM_REGISTERED and info.n_filtered == info.n_target == want.shape[0]
    same_bytes(c.stream_current_scan(), want)
    assert res.converged and res.final_error == 0.0              # the same scan twice
    c.close()


# ------------------------------------------------------------------ 2. local map
def big_pair(ctx):
    return LocalMap(ctx, LocalMapConfig(0.5, 100.0, 1 << 20)), lm.LocalMapRef(0.5, 100.0, 1 << 20)


@pytest.fixture(scope="module")
def lattice():
    scan = inputs.lattice_scan()
    assert scan.shape[0] > inputs.LMAP_ROWS
    scan.setflags(write=False)
    return scan


def test_local_map_past_one_grid_of_elements(ctx, lattice):
    """531,441 scan rows into an empty table (k_lmap_keys' second trip); 3,000 rows onto those residents (the second trip of
    k_lmap_marks and k_lmap_merge, on the resident side and on the scan's); a pose 95 m off, which evicts, keeps and drops."""
    dev, ref = big_pair(ctx)
    info = add_both(dev, ref, lattice, I4)
    assert info == dict(rows=len(lattice), inserted=len(lattice), evicted=0, dropped=0, merged=0)
    rng = np.random.default_rng(31)
    info = add_both(dev, ref, rng.uniform(-21.0, 21.0, size=(3000, 3)), I4)
    assert info["inserted"] > 0 and info["merged"] > 0 and info["evicted"] == 0
    assert info["rows"] - info["inserted"] + 3000 + 1 > inputs.LMAP_ROWS
    before = ref.size()
    info = add_both(dev, ref, rng.uniform(-80.0, 80.0, size=(6000, 3)), inputs.shifted(95.0))
    assert info["evicted"] > 0 and before - info["evicted"] > 0 and info["dropped"] > 0 and info["inserted"] > 0
    assert info["merged"] > 0                                    # the scan reaches back into the surviving residents
    dev.close()


LMAP_EDGES = [(520000, inputs.LMAP_ROWS), (520000, inputs.LMAP_ROWS + 1), (520000, inputs.LMAP_ROWS + 2),
              (0, inputs.LMAP_ROWS + 1), (0, inputs.LMAP_ROWS + 2)]


@pytest.mark.parametrize("resident,elements", LMAP_EDGES)
def test_local_map_at_the_grid_edge(ctx, lattice, resident, elements):
    """R residents and a scan of n rows with R + n + 1 = `elements`: k_lmap_marks runs over R + n + 1 elements and
    k_lmap_merge over R + n, so one grid's worth, one more and two more put the single element of a second trip at the end
    of the marks, then of the merge.  Without residents the scan is a prefix of the lattice: k_lmap_keys' n at the edge."""
    dev, ref = big_pair(ctx)
    n = elements - resident - 1
    if resident:
        assert add_both(dev, ref, lattice[:resident], I4)["rows"] == resident
        scan = np.random.default_rng(elements).uniform(-21.0, 21.0, size=(n, 3))
        info = add_both(dev, ref, scan, inputs.shifted(0.1, -0.2, 0.05))
        assert info["inserted"] > 0 and info["merged"] > 0
    else:
        assert n in (inputs.LMAP_ROWS, inputs.LMAP_ROWS + 1)
        assert add_both(dev, ref, lattice[:n], I4)["inserted"] == n
    dev.close()


# ------------------------------------------------------------------ 3. transform_points
@pytest.mark.parametrize("n", [inputs.GRID_ROWS, inputs.GRID_ROWS + 1, inputs.TRIP_ROWS, inputs.TRIP_ROWS + 1,
                               inputs.TRIP_ROWS + inputs.GRID_ROWS + 1])
def test_transform_points_past_the_grid(ctx, n):
    """one grid of rows and one more (the second row of a thread's batch), one trip of the loop and one more row (the second
    trip), and a second trip whose batch has a second row: every row is the unfused row-by-row product"""
    assert inputs.ROW_BATCH == 2 and n in (524288, 524289, 1048576, 1048577, 1572865)
    T, rows = inputs.transform_matrix(), inputs.transform_rows(n)
    same_bytes(ctx.transform_points(T, rows), inputs.moved_rows(T, rows))


# ------------------------------------------------------------------ 4. a registration past two grids of rows
@pytest.fixture(scope="module")
def long_registration(oracle):
    """source, target and the oracle's run: made once, shared, left unchanged"""
    src, tgt = inputs.registration_pair()
    assert src.shape[0] == 2 * inputs.GRID_ROWS + 1
    ref = oracle.icp_point_to_plane(src, tgt, max_iterations=3, tolerance=0.0, min_error=0.0, nthreads=8)
    assert not ref.converged and ref.num_iterations == 3 and len(ref.error_history) == 4
    src.setflags(write=False)
    tgt.setflags(write=False)
    return src, tgt, ref


def test_registration_past_two_grids_of_rows(gpu_ctx, long_registration):
    """1,048,577 source rows against 3,000 targets, three passes with the stopping tests off, on every engine, against the
    oracle within check_against's bounds (1e-4 m, 1e-4 rad, the history within 1e-9; reversing the source's rows moves the
    oracle's own history by 1e-15).

    The kernels that moved the rows, from the profile counters of the run on an MI355X (printed below): on every engine
    transform_launches == 1 -- the first move, k_transform with the Morton permutation on its 2048 x 256 grid, whose
    second trip holds the one row past 2 x 524,288 -- and reduce_launches == 4, the passes' sums, whose first three end in
    the fused mover (k_finish_step_transform on exact_f64 and mfma_bf16, k_finish_step_transform_cull on mfma_pruned:
    128 x 1024 threads, kRowBatch rows each, five trips); no unfused k_transform in the loop, small_launches == 0,
    nn_solo_passes == 0 (profile level 2 keeps the three-launch form).  nn_launches == 4 everywhere, bounded_launches ==
    coarse_launches == 4 on the two MFMA engines.  Measured there: pose 1.8e-16 m / 1.8e-18 rad from the oracle's, the
    history within 1.9e-15, on all three engines."""
    src, tgt, ref = long_registration
    before = gpu_ctx.get_profile()
    res, hist = gpu_ctx.align(src, tgt, capi.Context.make_config(3, 0.0, 0.0))
    after = gpu_ctx.get_profile()
    print("%s, %d rows:" % (gpu_ctx.engine, src.shape[0]),
          {k: after[k] - before[k] for k in after if k.endswith("_launches") or k.endswith("_passes")})
    dt, dr = check_against(res, hist, ref.transformation, ref.converged, ref.num_iterations, ref.error_history)
    print("pose delta %.2e m, %.2e rad; history delta %.2e" % (dt, dr, np.abs(hist - ref.error_history).max()))
