"""Plane-to-plane ICP off the device: the row arithmetic k_reduce_gicp includes as text
(csrc/icp_gicp_row.inc), compiled for the host with -ffp-contract=off (tests/cpp/gicp_row_host.cpp), gives
scripts/gicp_ref.py's 29 columns BIT FOR BIT on random rows and on the edge cases; the contract stands in the same words
in the C header, the kernel's header and the restatement; the C ABI's new structs have the layout the ctypes mirrors
assume and the existing ones keep theirs; the C++ mirror compiles clean."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import gicp_ref as ref  # noqa: E402

dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the row arithmetic as the host compiler builds it, unfused"""
    so = tmp_path_factory.mktemp("gicp") / "libgicp_row_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "gicp_row_host.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.gicp_row_columns.argtypes = [dp, dp, dp, dp, C.c_long, C.c_double, C.c_double, dp]
    lib.gicp_row_columns.restype = None
    lib.gicp_rotate_normal.argtypes = [dp, dp, dp]
    lib.gicp_rotate_normal.restype = None
    return lib


def _ptr(a):
    return a.ctypes.data_as(dp)


def _host_columns(lib, p, q, n, m, c, kappa):
    p, q, n, m = (np.ascontiguousarray(a, dtype=np.float64) for a in (p, q, n, m))
    out = np.full((p.shape[0], 29), np.nan)
    lib.gicp_row_columns(_ptr(p), _ptr(q), _ptr(n), _ptr(m), p.shape[0], c, kappa, _ptr(out))
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _unit(rng, rows):
    v = rng.normal(size=(rows, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _same(lib, p, q, n, m, epsilon):
    c, kappa = 1.0 - epsilon, 2.0 * epsilon
    want = ref.gicp_row_columns(p, q, n, m, c, kappa)
    got = _host_columns(lib, p, q, n, m, c, kappa)
    assert np.isfinite(want).all()
    assert np.array_equal(_bits(got), _bits(want))
    return want


@pytest.mark.parametrize("epsilon", [1e-3, 0.25, 1.0])
def test_random_rows_bit_for_bit(host, epsilon):
    rng = np.random.default_rng(2024)
    p = rng.uniform(-60.0, 60.0, size=(1000, 3))
    q = p + rng.normal(0.0, 0.3, size=p.shape)
    cols = _same(host, p, q, _unit(rng, 1000), _unit(rng, 1000), epsilon)
    assert (cols[:, 28] == 1.0).all() and (cols[:, 27] >= 0.0).all()


def test_edge_cases_bit_for_bit(host):
    rng = np.random.default_rng(7)
    p = rng.uniform(-40.0, 40.0, size=(64, 3))
    q = p + rng.normal(0.0, 0.2, size=p.shape)
    n = _unit(rng, 64)
    t = np.cross(n, _unit(rng, 64))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    for epsilon in (1e-3, 1.0):
        _same(host, p, q, n, n.copy(), epsilon)                      # n parallel to m
        _same(host, p, q, n, -n, epsilon)                            # ... and antiparallel
        _same(host, p, q, n, t, epsilon)                             # n perpendicular to m
        cols = _same(host, np.zeros_like(p), q - p, n, t, epsilon)   # p = 0: no rotation rows, no lever
        assert (cols[:, :15] == 0.0).all() and (cols[:, 21:24] == 0.0).all()
    # axis-aligned normals, exactly representable: M is diagonal
    ez = np.tile([0.0, 0.0, 1.0], (64, 1))
    cols = _same(host, p, q, ez, ez, 0.5)
    assert (cols[:, 15] == 0.5).all() and (cols[:, 18] == 0.5).all() and (cols[:, 20] == 1.0).all()   # 1/2, 1/2, 1/(2 eps)


def test_epsilon_one_is_point_to_point_exactly(host):
    """S = 2 I and M = I / 2 to the bit, whatever the normals"""
    rng = np.random.default_rng(11)
    p = rng.uniform(-40.0, 40.0, size=(200, 3))
    q = p + rng.normal(0.0, 0.2, size=p.shape)
    cols = _same(host, p, q, _unit(rng, 200), _unit(rng, 200), 1.0)
    assert (cols[:, [15, 18, 20]] == 0.5).all() and (cols[:, [16, 17, 19]] == 0.0).all()
    e = q - p
    assert np.array_equal(cols[:, 24:27], 0.5 * e)
    assert np.array_equal(cols[:, 27], 2.0 * ((e[:, 0] * (0.5 * e[:, 0]) + e[:, 1] * (0.5 * e[:, 1])) + e[:, 2] * (0.5 * e[:, 2])))


def test_parallel_normals_read_in_metres(host):
    """kappa e^T M e = (e.n)^2 + epsilon * (tangential)^2 when n == m (to rounding: a tolerance from the condition 1/eps)"""
    rng = np.random.default_rng(3)
    p = rng.uniform(-40.0, 40.0, size=(500, 3))
    e = rng.normal(0.0, 0.2, size=p.shape)
    n = _unit(rng, 500)
    epsilon = 1e-3
    cols = _same(host, p, p + e, n, n.copy(), epsilon)
    en = (e * n).sum(axis=1)
    want = en * en + epsilon * ((e * e).sum(axis=1) - en * en)
    assert np.allclose(cols[:, 27], want, rtol=1e-9, atol=0.0)


def test_the_normal_equations_are_the_point_to_plane_ones_in_the_limit(host):
    """A^T M A and A^T M e against dense numpy, and against J J^T / J b with M = n n^T put in by hand"""
    rng = np.random.default_rng(5)
    p = rng.uniform(-40.0, 40.0, size=(50, 3))
    e = rng.normal(0.0, 0.2, size=p.shape)
    n, m = _unit(rng, 50), _unit(rng, 50)
    epsilon = 0.01
    cols = _same(host, p, p + e, n, m, epsilon)
    for i in range(50):
        px = np.array([[0.0, -p[i, 2], p[i, 1]], [p[i, 2], 0.0, -p[i, 0]], [-p[i, 1], p[i, 0], 0.0]])
        A = np.hstack([-px, np.eye(3)])
        S = 2.0 * np.eye(3) - (1.0 - epsilon) * (np.outer(n[i], n[i]) + np.outer(m[i], m[i]))
        M = np.linalg.inv(S)
        H, g = ref.normal_matrix(cols[i])
        assert np.allclose(H, A.T @ M @ A, rtol=1e-9, atol=1e-9)
        assert np.allclose(g, A.T @ M @ e[i], rtol=1e-9, atol=1e-9)
        J = np.concatenate([np.cross(p[i], n[i]), n[i]])
        assert np.allclose(A.T @ np.outer(n[i], n[i]) @ A, np.outer(J, J), rtol=1e-12, atol=1e-9)


def test_the_rotation_bit_for_bit(host):
    rng = np.random.default_rng(9)
    for _ in range(20):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        T = np.eye(4)
        T[:3, :3] = q
        T[:3, 3] = rng.normal(size=3)
        s = _unit(rng, 1)
        got = np.full(3, np.nan)
        host.gicp_rotate_normal(_ptr(np.ascontiguousarray(T)), _ptr(np.ascontiguousarray(s)), _ptr(got))
        assert np.array_equal(_bits(got), _bits(ref.rotate_normals(T, s)[0]))


# ------------------------------------------------------------------------------------------------ the three statements

def _contract(path, first, last):
    """the contract's lines of a file, comment marks and indentation stripped"""
    lines = open(path).read().splitlines()
    strip = [re.sub(r"^\s*(//|\*|/\*)?\s*", "", ln).rstrip() for ln in lines]
    a = next(k for k, ln in enumerate(strip) if ln.startswith(first))
    b = next(k for k, ln in enumerate(strip) if k > a and ln.startswith(last))
    return [ln for ln in strip[a:b + 1] if ln]


def test_the_contract_is_stated_in_the_same_words_three_times():
    first, last = "R    = rotation block", "28      1.0"
    texts = [_contract(p, first, last) for p in (os.path.join(INCLUDE, "icp_mi355x.h"), os.path.join(CSRC, "icp_gicp.h"),
                                                  os.path.join(ROOT, "scripts", "gicp_ref.py"))]
    assert len(texts[0]) == 24
    formulas = [[ln for ln in t if not ln.startswith("Columns of a kept row")] for t in texts]   # (its parenthesis names the sibling)
    assert formulas[0] == formulas[1] == formulas[2]
    for path in (os.path.join(INCLUDE, "icp_mi355x.h"), os.path.join(CSRC, "icp_gicp.h"), os.path.join(ROOT, "scripts", "gicp_ref.py")):
        text = open(path).read()
        assert "metres" in text and "point-to-point" in text


# ------------------------------------------------------------------------------------------------ the ABI

def test_the_header_is_plain_c_and_the_structs_have_their_layout():
    probe = ('#include <stddef.h>\n#include "icp_mi355x.h"\n'
             '_Static_assert(sizeof(icpmi_gicp) == 24 && offsetof(icpmi_gicp, epsilon) == 0 && offsetof(icpmi_gicp, max_distance) == 8\n'
             '               && offsetof(icpmi_gicp, reserved) == 16, "icpmi_gicp");\n'
             '_Static_assert(sizeof(icpmi_gicp_info) == 16 && offsetof(icpmi_gicp_info, rows) == 8, "icpmi_gicp_info");\n'
             '_Static_assert(sizeof(icpmi_config) == 152 && sizeof(icpmi_result) == 152 && sizeof(icpmi_gate) == 16\n'
             '               && sizeof(icpmi_gate_info) == 16 && sizeof(icpmi_robust) == 24 && sizeof(icpmi_robust_info) == 24\n'
             '               && sizeof(icpmi_stream_info) == 24 && sizeof(icpmi_normal_matrix) == 488, "the existing structs");\n'
             'int main(void) {\n'
             '    icpmi_gicp r = {ICPMI_GICP_EPSILON_DEFAULT, 2.0, 0}; icpmi_gicp_info i = {0, 0};\n'
             '    int (*a)(icpmi_ctx *, const double *, int64_t, const double *, int64_t, const icpmi_config *, const icpmi_gicp *,\n'
             '             icpmi_result *, icpmi_gicp_info *, double *, int32_t) = icpmi_align_gicp;\n'
             '    int (*b)(icpmi_ctx *, const double *, int64_t, const double *, int64_t, const icpmi_config *, const icpmi_gicp *,\n'
             '             icpmi_result *, icpmi_gicp_info *, double *, int32_t) = icpmi_align_gicp_device;\n'
             '    return (int)(r.epsilon + (double)i.pairs) * 0 + (a && b ? 0 : 1);\n'
             '}\n')
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-x", "c", "-"],
                   input=probe, text=True, check=True)


def test_the_cpp_mirror_is_clean_cpp17():
    probe = ('#include "icp_mi355x.hpp"\n'
             'int main() {\n'
             '    icp_mi355x::GicpRule rule;\n'
             '    rule.max_distance = 2.0;\n'
             '    icp_mi355x::GicpICPResult (*f)(icp_mi355x::Context &, const double *, std::size_t, const double *, std::size_t,\n'
             '                              const icp_mi355x::GicpRule &, const icp_mi355x::ICPConfig &) = &icp_mi355x::align_gicp;\n'
             '    icp_mi355x::GicpICPResult (*g)(const icp_mi355x::PointCloud &, const icp_mi355x::PointCloud &, const icp_mi355x::GicpRule &,\n'
             '                              const icp_mi355x::ICPConfig &) = &icp_mi355x::align_gicp;\n'
             '    icp_mi355x::GicpICPResult out;\n'
             '    return rule.epsilon == ICPMI_GICP_EPSILON_DEFAULT && f && g && out.pairs == 0 ? 0 : 1;\n'
             '}\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-x", "c++", "-"],
                   input=probe, text=True, check=True)


def test_ctypes_mirrors_agree():
    from lidar_slam_from_scratch_amd import capi
    assert C.sizeof(capi.Gicp) == 24 and C.sizeof(capi.GicpInfo) == 16
    assert (capi.Gicp.epsilon.offset, capi.Gicp.max_distance.offset, capi.Gicp.reserved.offset) == (0, 8, 16)
    assert (capi.GicpInfo.pairs.offset, capi.GicpInfo.rows.offset) == (0, 8)
    assert capi.GICP_EPSILON_DEFAULT == ref.EPSILON_DEFAULT == 1e-3
    assert C.sizeof(capi.Config) == 152 and C.sizeof(capi.Result) == 152 and C.sizeof(capi.Robust) == 24
    for name in ("icpmi_align_gicp", "icpmi_align_gicp_device"):
        assert name in capi.EXPORTS
    g = capi.as_gicp((1e-3, 2.0))
    assert (g.epsilon, g.max_distance) == (1e-3, 2.0) and capi.as_gicp(g) is g
    assert capi.as_gicp((0.5,)).max_distance == 0.0


def test_the_plan_of_a_plane_to_plane_call(tmp_path):
    """kRuleGicp: neither fused nor small at any size, every other path off, reduce_blocks() partial rows and no group
    sums -- through tests/cpp/loop_plan_print.cpp's sibling, a probe compiled here"""
    probe = ('#include <cstdio>\n#include "loop_plan.h"\nusing namespace icpmi;\n'
             'int main() {\n'
             '    int bad = 0;\n'
             '    const int engines[] = {ICPMI_SEARCH_EXACT_F64, ICPMI_SEARCH_MFMA_BF16};\n'
             '    for (int engine : engines) for (int pruned = 0; pruned < 2; ++pruned)\n'
             '    for (int n : {1, 5, 33, 1001, 8799, 32768, 65537, 1000000}) for (int splits : {1, 4, 8, 9, 13, 49, 500}) {\n'
             '        LoopFacts f; f.n = n; f.m = splits * 2048; f.nn_engine = engine; f.nn_pruned = pruned && engine == ICPMI_SEARCH_MFMA_BF16;\n'
             '        f.nn_splits = splits; f.rule = kRuleGicp;\n'
             '        const LoopPlan p = make_loop_plan(f);\n'
             '        LoopFacts g = f; g.rule = kRuleGate;\n'
             '        const LoopPlan q = make_loop_plan(g);\n'
             '        const bool ok = p.rule == kRuleGicp && !p.fused && !p.small && !p.pruned && !p.sorted_rows_loop && !p.sort_source &&\n'
             '            !p.bounded && !p.reuse && !p.margin && !p.lean_on && !p.fused_tail && !p.cull_full && !p.sum_tree && !p.error &&\n'
             '            p.rblocks == reduce_blocks(f.cu_count, n) && p.fin_blocks == p.rblocks && p.rblocks2 == 0 &&\n'
             '            (q.small || (q.rblocks == p.rblocks && q.fin_blocks == p.fin_blocks));\n'
             '        if (!ok) { std::printf("n %d splits %d engine %d\\n", n, splits, engine); ++bad; }\n'
             '    }\n'
             '    return bad ? 1 : 0;\n'
             '}\n')
    exe = str(tmp_path / "gicp_plan_probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-x", "c++", "-", "-o", exe],
                   input=probe, text=True, check=True)
    subprocess.check_call([exe])
