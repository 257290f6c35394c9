"""scripts/fuzz_loop_rows.py's exact_nn -- the reference every pass of the ICP loop is checked against
(tests/test_gpu_loop_matches.py) -- against the oracle's brute force (strict < in index order: ties go to the lowest
index, non-finite targets never match) where a kd-tree's candidates are easiest to get wrong: exact ties, duplicates,
large offsets, non-finite rows.  Runs on the CPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def _lattice(side, rng, n_dup):
    g = np.stack(np.meshgrid(*[np.arange(side, dtype=np.float64)] * 3, indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(g.shape[0])]
    dup = rng.choice(g.shape[0], n_dup, replace=False)
    g[dup] = g[rng.integers(0, g.shape[0], n_dup)]
    return np.ascontiguousarray(g)


def _cases():
    rng = np.random.default_rng(77)
    t = _lattice(14, rng, 300)
    q = t[rng.integers(0, t.shape[0], 1500)] + rng.integers(-1, 2, (1500, 3)) * 0.5    # on, between and beside the points
    yield "lattice_duplicates", t, q
    # a shifted sub-lattice: every row is equidistant from four targets (eight where the duplicates double them)
    s = np.stack(np.meshgrid(np.arange(13) + 0.5, np.arange(13) + 0.5, np.arange(14.0), indexing="ij"), -1).reshape(-1, 3)
    yield "sub_lattice", t, np.ascontiguousarray(s)
    t2 = rng.uniform(-1, 1, (3000, 3)) * 20 + 1e5
    q2 = rng.uniform(-1, 1, (2000, 3)) * 22 + 1e5
    q2[:300] = t2[rng.choice(3000, 300, replace=False)]
    yield "offset_1e5", t2, q2
    t3 = _lattice(10, rng, 50) + 1e5
    yield "offset_1e5_lattice", t3, t3[rng.integers(0, t3.shape[0], 800)] + np.array([0.5, 0.5, 0.0])
    t4 = rng.uniform(-1, 1, (2500, 3))
    q4 = rng.uniform(-1.2, 1.2, (1200, 3))
    t4[rng.choice(2500, 40, replace=False)] = np.nan
    t4[rng.choice(2500, 30, replace=False), 1] = np.inf
    t4[rng.choice(2500, 30, replace=False), 2] = -np.inf
    q4[::37] = np.nan
    q4[5::41, 0] = np.inf
    q4[7::43, 2] = -np.inf
    yield "nonfinite", t4, q4
    yield "all_targets_nonfinite", np.full((5, 3), np.nan), q4[:50]
    yield "one_target", t4[~np.isnan(t4).any(axis=1) & np.isfinite(t4).all(axis=1)][:1], q4


@pytest.mark.parametrize("name", [c[0] for c in _cases()])
def test_exact_nn_matches_brute_force(name, oracle):
    import fuzz_loop_rows
    t, q = next((t, q) for n, t, q in _cases() if n == name)
    want, _ = oracle.nearest_batch_brute(t, q)
    got = fuzz_loop_rows.exact_nn(t, q)
    assert got.dtype == np.int64 and got.shape == (q.shape[0],)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(r), int(got[r]), int(want[r])) for r in bad[:10]]
    assert ((want >= 0) == np.isfinite(q).all(axis=1) if np.isfinite(t).all(axis=1).any() else (want < 0)).all()


def test_exact_nn_ties_go_to_the_lowest_index(oracle):
    """The sub-lattice rows really are ties (four targets at 0.5), so the case above tests the tie rule, and a
    duplicate of a target always loses to the earlier copy."""
    import fuzz_loop_rows
    t = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [1, 1, 0], [0, 0, 0]])
    q = np.array([[0.5, 0.5, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 0.0], [0.9, 0.5, 0.0]])
    assert fuzz_loop_rows.exact_nn(t, q).tolist() == [0, 3, 0, 1]
    d2 = fuzz_loop_rows.sqdist(t, q[0])
    assert (d2[:5] == 0.5).all()


def test_error_bound_separates_one_wrong_match():
    """(b)'s tolerance: one row matched with the second-nearest target moves the recomputed error by far more than the
    bound on re-ordering the sum, at the sizes of the GPU cases."""
    import fuzz_loop_rows
    rng = np.random.default_rng(5)
    t = rng.uniform(-10, 10, (20000, 3))
    nrm = rng.normal(size=(20000, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    cur = rng.uniform(-10, 10, (40000, 3))
    idx = fuzz_loop_rows.exact_nn(t, cur)
    terms = fuzz_loop_rows.plane_terms(cur, t, nrm, idx)
    e0 = np.sqrt(np.sum(terms) / cur.shape[0])
    e1 = np.sqrt(np.sum(terms[::-1]) / cur.shape[0])
    assert abs(e0 - e1) <= fuzz_loop_rows.error_bound(cur.shape[0]) * e0
    # the rows whose second-nearest target changes their term the most and the least (of the first 200)
    from scipy.spatial import cKDTree
    _, j2 = cKDTree(t).query(cur[:200], k=2)
    moved = []
    for r in range(200):
        wrong = idx.copy()
        wrong[r] = j2[r, 1] if j2[r, 0] == idx[r] else j2[r, 0]
        e2 = np.sqrt(np.sum(fuzz_loop_rows.plane_terms(cur, t, nrm, wrong)) / cur.shape[0])
        moved.append(abs(e2 - e0) / e0)
    assert np.median(moved) > 1e3 * fuzz_loop_rows.error_bound(cur.shape[0])
