"""The exact-sum fixtures of scripts/exact_lattice.py under the CPU oracle alone (no GPU): every condition that
tests/test_gpu_exact_sums.py relies on when it holds the device's sums to an integer reference bit for bit.

  * the oracle's normals of the lattice targets are exact axis vectors, its matches the constructed ones;
  * the float sums (the oracle's loop in index order, the same loop in reversed order, numpy's matrix product) equal the
    integer sums to the bit, and the bound that makes this so -- a column's absolute terms add up to less than 2^53 in
    the column's unit -- holds;
  * the gate keeps exactly the rows at and inside d^2 == g^2 and the weights are exactly 1, 1/2 and 1/4 under the CPU
    restatements scripts/gated_icp_ref.py and scripts/robust_icp_ref.py;
  * the hand-made 6 x 6 systems do what they were made for under the oracle, and the oracle's solve equals the
    reference's own Eigen build bit for bit where oracle/ref_hook.cpp can be built (skipped where it cannot, as in
    tests/test_reference_hook.py);
  * tests/cpp/loop_plan_print.cpp, which gives the GPU test its source sizes, builds and reaches the edges."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import exact_lattice as xl  # noqa: E402

# (patches, source rows): the small-cloud target and the 15-split target of the GPU test, the latter at its largest
# source (the offsets of the table that 131,089 rows reach)
TARGETS = {"3_patches": (3, 2 * 4800 + 77), "18_patches": (18, 131089)}
_made = {}


def made(name, oracle):
    """target, the oracle's tree and normals: computed once, shared, left unchanged"""
    if name not in _made:
        t = xl.target(TARGETS[name][0])
        tree = oracle.KDTree(t.pts)
        _made[name] = (t, tree, oracle.estimate_normals(t.pts, tree, 20, nthreads=4))
    return _made[name]


def same_bits(a, b):
    """equal values, none of them a NaN (for finite non-zero doubles: equal bits; +0 and -0 are one value)"""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


@pytest.mark.parametrize("name", list(TARGETS))
def test_oracle_normals_are_axis_vectors(oracle, name):
    t, _tree, nrm = made(name, oracle)
    assert same_bits(np.abs(nrm), xl.axis_normals(t.axis))


@pytest.mark.parametrize("kind", ["plain", "gate", "huber", "gm", "step"])
@pytest.mark.parametrize("name", list(TARGETS))
def test_matches_and_sums(oracle, name, kind):
    t, tree, nrm = made(name, oracle)
    n = TARGETS[name][1] if kind != "gate" else 10 * 4800 + 13       # (every offset of the gate's table)
    if name == "18_patches" and kind != "plain":
        n = 28800 + 4099
    s, keep, w4, want = xl.variant(kind, t, n)
    idx, d2 = tree.nearest_batch(s.pts, nthreads=4)
    assert np.array_equal(idx, s.match)
    assert want.largest < 2 ** 53 and want.pairs == int(keep.sum())
    p, q, nn = s.pts[keep], t.pts[idx[keep]], nrm[idx[keep]]
    w = w4[keep] / 4.0
    J = np.concatenate([np.cross(p, nn), nn], axis=1)
    b = np.sum((q - p) * nn, axis=1)
    assert same_bits((w[:, None] * J).T @ J, want.JtJ)
    assert same_bits((w[:, None] * J).T @ b, want.Jtb)
    assert same_bits(np.sum(w * b * b), want.sum_sq) and float(np.sum(w)) == want.weight
    if kind in ("plain", "step"):                                    # the oracle's own loop, and the same loop backwards
        assert same_bits(oracle.normal_equations(p, q, nn), want.sums28())
        assert same_bits(oracle.normal_equations(p[::-1], q[::-1], nn[::-1]), want.sums28())
    if kind == "gate":                                               # at the gate: in; one representable number beyond: out
        at = keep & (np.abs(np.linalg.norm(s.off, axis=1) - xl.GATE) == 0.0)
        assert at.sum() > n // 4 and (d2[at] == xl.GATE * xl.GATE).all()
        assert s.outside.sum() > n // 5 and (d2[s.outside] > xl.GATE * xl.GATE).all()
        assert (d2[keep] <= xl.GATE * xl.GATE).all()


def test_plain_lattice_solves_to_its_offset(oracle):
    t, tree, nrm = made("3_patches", oracle)
    s = xl.source(t, len(t.pts), xl.PLAIN_OFFSETS[:1])
    T = oracle.solve_point_to_plane(s.pts, t.pts, nrm)
    # (the sums are exact, the factorisation's divisions are not: the translation comes back to a few ulps, and the
    # rotation, 1e-17, takes the identity branch of the step)
    assert same_bits(T[:3, :3], np.eye(3)) and np.abs(T[:3, 3] + xl.PLAIN_OFFSETS[0]).max() < 1e-15


def test_cyclic_fixture_ties_the_diagonals(oracle):
    t = xl.target(3, cyclic=True)
    tree = oracle.KDTree(t.pts)
    nrm = oracle.estimate_normals(t.pts, tree, 20, nthreads=4)
    assert same_bits(np.abs(nrm), xl.axis_normals(t.axis))
    s, _keep, _w4, want = xl.variant("cyclic_step", t, len(t.pts))
    idx, _d2 = tree.nearest_batch(s.pts, nthreads=4)
    assert np.array_equal(idx, s.match) and want.largest < 2 ** 53
    assert same_bits(oracle.normal_equations(s.pts, t.pts[idx], nrm[idx]), want.sums28())
    d = np.diag(want.JtJ)
    assert d[0] == d[1] == d[2] > d[3] == d[4] == d[5] > 0.0         # both blocks tied ...
    assert len(set(want.Jtb)) == 6                                   # ... and a right-hand side without symmetry
    T = oracle.solve_point_to_plane(s.pts, t.pts[idx], nrm[idx])
    assert 1e-3 < math.acos((np.trace(T[:3, :3]) - 1.0) / 2.0) < 0.1


def test_gate_under_the_restatement(oracle):
    import gated_icp_ref as gr
    t, tree, nrm = made("3_patches", oracle)
    s, keep, _w4, want = xl.variant("gate", t, 10 * 4800 + 13)
    r = gr.gated_icp(s.pts, t.pts, xl.GATE, max_iterations=0, orc=oracle, normals=nrm, tree=tree)
    assert r.pairs == want.pairs == int(keep.sum()) and r.min_margin == 0.0
    assert r.final_error == math.sqrt(want.sum_sq / want.weight)


@pytest.mark.parametrize("kind", ["huber", "gm"])
def test_weights_under_the_restatement(oracle, kind):
    import robust_icp_ref as rr
    t, tree, nrm = made("3_patches", oracle)
    n = 8 * 4800 + 13
    s, keep, w4, want = xl.variant(kind, t, n)
    code, k = (rr.HUBER, xl.HUBER_K) if kind == "huber" else (rr.GEMAN_MCCLURE, xl.GM_K)
    q, nn = t.pts[s.match], nrm[s.match]
    b = np.sum((q - s.pts) * nn, axis=1)
    assert same_bits(rr.weights(code, k, b), w4 / 4.0)
    assert set(np.unique(w4)) == ({1, 2, 4} if kind == "huber" else {1, 4})
    if kind == "gm":                                                 # the formula's intermediates, step by step
        sc = k * k
        tt = sc + b * b
        assert set(np.unique(tt / sc)) == {1.0, 2.0} and set(np.unique(sc / tt)) == {1.0, 0.5}
    sums = rr.weighted_sums(s.pts, q, nn, code, k)
    assert same_bits(sums[:28], want.sums28()) and sums[28] == want.weight and sums[29] == want.pairs
    r = rr.robust_icp(s.pts, t.pts, code, k, max_iterations=0, orc=oracle, normals=nrm, tree=tree)
    assert r.weight_sum == want.weight and r.pairs == n
    assert r.final_error == math.sqrt(want.sum_sq / want.weight)


def test_hand_made_systems_under_the_oracle(oracle):
    systems = xl.hand_made_systems()
    for name, (src, tgt, nrm, expect) in systems.items():
        T = oracle.solve_point_to_plane(src, tgt, nrm)
        sums = oracle.normal_equations(src, tgt, nrm)
        if expect == "nan":
            assert np.isnan(sums).any() and np.isnan(T).any(), name
            continue
        assert same_bits(sums, oracle.normal_equations(src[::-1], tgt[::-1], nrm[::-1])), name   # exact in any order
        assert np.isfinite(T).all(), name
        if expect == "identity":
            assert same_bits(T, np.eye(4)) and not sums.any(), name
    # what each system was made for
    s = {k: oracle.normal_equations(*v[:3]) for k, v in systems.items()}
    diag = [0, 6, 11, 15, 18, 20]                                    # the diagonal's places among the 21 entries
    assert len(set(s["full_rank_ties"][diag[:3]])) == 1 and len(set(s["full_rank_ties"][diag[3:]])) == 1
    J = {k: np.concatenate([np.cross(v[0], v[2]), v[2]], axis=1) for k, v in systems.items() if v[3] == "oracle"}
    assert np.linalg.matrix_rank(J["full_rank_ties"]) == 6 and np.linalg.matrix_rank(J["rank3_one_patch"]) == 3
    assert np.linalg.matrix_rank(J["rank2_line"]) == 2 and np.linalg.matrix_rank(J["rank1_one_row"]) == 1
    # the pseudo-inverse rule.  xl.ldlt6_solve restates the oracle's solve with the rule's threshold as a parameter: with
    # DBL_MIN it gives the oracle's translation bit for bit on every system; with 0.0 -- a plain division -- it gives
    # another answer on the two systems made for the rule, whose right-hand sides are not zero
    for name, (src, tgt, nrm, expect) in systems.items():
        if expect != "nan":
            x, _pivots = xl.ldlt6_solve(*xl.sums_to_system(s[name]), sys.float_info.min)
            assert same_bits(x[3:], oracle.solve_point_to_plane(src, tgt, nrm)[:3, 3]), name
    for name, ruled, solved in (("normals_2^-540", 6, 0), ("normals_2^-513", 3, 3)):
        M, rhs = xl.sums_to_system(s[name])
        assert rhs.all(), (name, rhs)                                # Jtb survives, every entry
        x_rule, pivots = xl.ldlt6_solve(M, rhs, sys.float_info.min)
        x_plain, _pivots = xl.ldlt6_solve(M, rhs, 0.0)
        assert int((np.abs(pivots) <= sys.float_info.min).sum()) == ruled and (pivots[:3] > 0.0).all(), (name, pivots)
        assert int((x_rule != 0.0).sum()) == solved and not same_bits(x_rule, x_plain), (name, x_rule, x_plain)
        assert np.abs(x_plain[:3] - x_rule[:3]).max() > 1e-4, (name, x_rule, x_plain)   # far beyond the rotation's bound
        T = oracle.solve_point_to_plane(*systems[name][:3])
        assert same_bits(T, np.eye(4)) == (solved == 0), (name, T)
    assert xl.rotation_norm(*systems["under_pi_4"][:3]) < math.pi / 4 < xl.rotation_norm(*systems["over_pi_4"][:3])
    assert abs(xl.rotation_norm(*systems["under_pi_4"][:3]) - math.pi / 4) < 2e-3
    assert abs(xl.rotation_norm(*systems["over_pi_4"][:3]) - math.pi / 4) < 2e-3
    T = oracle.solve_point_to_plane(*systems["below_1e-10"][:3])
    assert 0.0 < xl.rotation_norm(*systems["below_1e-10"][:3]) < 1e-10 and same_bits(T[:3, :3], np.eye(3)) and T[:3, 3].any()


def test_hand_made_systems_against_the_reference(oracle):
    if oracle.ref_lib() is None:
        pytest.skip("the reference cannot be built here (needs Eigen3 and a reference checkout): `make -C oracle ref`")
    for name, (src, tgt, nrm, expect) in xl.hand_made_systems().items():
        T_ref = oracle.ref_solve_point_to_plane(src, tgt, nrm)
        T_orc = oracle.solve_point_to_plane(src, tgt, nrm)
        if expect == "nan":
            assert np.array_equal(np.isnan(T_ref), np.isnan(T_orc)), name
        else:
            assert same_bits(T_orc, T_ref), (name, T_orc, T_ref)


def test_plan_printer_covers_the_edges(tmp_path):
    """tests/cpp/loop_plan_print.cpp, which the GPU test takes its source sizes from: it builds without warnings, its runs
    tile the sizes asked for without a gap, and on the small-cloud path (one partial row per 32 rows up to 32,768) they
    reach every edge of finish_sums and the sum tree's threshold."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "loop_plan_print")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "loop_plan_print.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "engine=mfma", "splits=3", "cu=256", "n=1:40000"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    min_queries, small_max, group, tree_from = (int(v) for v in lines[0].split()[1:])
    runs = [tuple(int(v) for v in ln.split()) for ln in lines[1:]]
    assert runs[0][0] == 1 and runs[-1][1] == 40000 and all(b[0] == a[1] + 1 for a, b in zip(runs, runs[1:]))
    small = [run for run in runs if run[6]]
    assert small[-1][1] == small_max and all(not run[6] for run in runs if run[0] > small_max)
    assert {run[5] for run in small if not run[3]} >= {1, 127, 128, 129, 256, 257, 512, 513}
    assert all(bool(run[3]) == (run[2] >= tree_from) and run[4] == (-(-run[2] // group) if run[3] else 0) for run in runs)
    bad = subprocess.run([exe, "engine=triton"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2
