"""The inputs of tests/test_gpu_loop_trips.py (tests/loop_trip_inputs.py) do what they are there for, on the CPU: the dense
cloud has the run lengths around the 64-row chunk of k_voxel_centroids and its rows sit off the cell faces; the oracle's
centroids are the sequential sums, and a kernel that summed a chunk before adding it would NOT reproduce them; the sizes
are past the grids' caps as the headers state them."""
import numpy as np

import loop_trip_inputs as inputs


def test_thresholds_from_the_headers():
    assert inputs.LMAP_ROWS == 524288 and inputs.GRID_ROWS == 524288 and inputs.ROW_BATCH == 2
    assert inputs.LATTICE_SIDE ** 3 == 531441 > inputs.LMAP_ROWS
    assert inputs.REGISTRATION_ROWS == 2 * 2048 * 256 + 1


def test_dense_cloud_runs_and_margins():
    pts, cells = inputs.dense_cloud()
    assert pts.shape == (sum(inputs.RUNS), 3) == (7378, 3)
    assert len({tuple(c) for c in inputs.dense_cells().tolist()}) == len(inputs.RUNS)
    assert (inputs.dense_cells().min(axis=0) < 0).all()
    q = pts / inputs.VOXEL
    assert np.array_equal(np.floor(q).astype(np.int64), cells)
    frac = q - np.floor(q)
    assert frac.min() >= 0.02 - 1e-12 and frac.max() <= 0.98 + 1e-12
    _, counts = inputs.centroids_by_loop(pts, inputs.VOXEL)
    assert sorted(counts) == sorted(inputs.RUNS)
    # scattered: a voxel's rows are not neighbours in the input (the 5,000-row voxel holds two rows of three)
    big = np.flatnonzero((cells == inputs.dense_cells()[-1]).all(axis=1))
    assert len(big) == 5000 and big.max() - big.min() > 7000 and (np.diff(big) > 1).sum() > 1000
    # full mantissa: the low bits of the rows are not all zero
    assert (pts.view(np.uint64) & np.uint64(0xFF)).astype(bool).mean() > 0.9


def test_oracle_is_the_sequential_sum_and_chunked_sums_are_not(oracle):
    pts, _ = inputs.dense_cloud()
    for cloud in (pts, np.ascontiguousarray(pts[::-1])):
        want, counts = inputs.centroids_by_loop(cloud, inputs.VOXEL)
        got = oracle.voxel_downsample(cloud, inputs.VOXEL)
        assert got.shape == want.shape and got.tobytes() == want.tobytes()
        chunked, _ = inputs.centroids_by_loop(cloud, inputs.VOXEL, chunk=inputs.CHUNK)
        counts = np.array(counts)
        differs = (chunked != want).any(axis=1)
        assert not differs[counts <= inputs.CHUNK].any()                     # one chunk: the same additions
        dense = counts > inputs.CHUNK
        assert dense.sum() == 10 and 2 * differs[dense].sum() >= dense.sum(), (differs[dense].sum(), dense.sum())
    fwd = inputs.centroids_by_loop(pts, inputs.VOXEL)[0]
    assert (fwd != want).any()                                               # reversing the rows changes the sums


def test_lattice_scan_is_one_row_per_voxel():
    scan = inputs.lattice_scan()
    assert scan.shape == (inputs.LATTICE_SIDE ** 3, 3)
    c = np.floor(scan / inputs.VOXEL).astype(np.int64) + 64
    keys = (c[:, 0] << 14) | (c[:, 1] << 7) | c[:, 2]
    assert len(np.unique(keys)) == len(scan) and -20.0 < scan.min() and scan.max() < 20.5     # cells -40 .. 40
    assert (np.diff(keys) < 0).sum() > len(scan) // 4                       # shuffled: the sort has work to do


def test_moved_rows_is_row_by_row():
    T, rows = inputs.transform_matrix(), inputs.transform_rows(257)
    assert not np.isin(T[:3], (0.0, 1.0)).any()
    got = inputs.moved_rows(T, rows)
    for i in (0, 128, 256):
        x, y, z = (float(v) for v in rows[i])
        for r in range(3):
            assert got[i, r] == ((x * float(T[r, 0]) + y * float(T[r, 1])) + z * float(T[r, 2])) + float(T[r, 3])
