"""The robust weights' C++ mirror compiles clean from a plain C++17 program, the new declarations are there, and the C
ABI's existing structs keep their layout: tests/cpp/robust_demo.cpp holds sizeof / offsetof static assertions on
icpmi_config, icpmi_result, icpmi_gate, icpmi_gate_info and icpmi_stream_info with the values they had before the weights
existed, and on the two new structs; the ctypes mirrors agree."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def test_robust_demo_is_clean_cpp17_and_the_structs_keep_their_layout():
    src = os.path.join(ROOT, "tests", "cpp", "robust_demo.cpp")
    text = open(src).read()
    for pinned in ("sizeof(icpmi_config) == 152", "sizeof(icpmi_result) == 152", "sizeof(icpmi_gate) == 16",
                   "sizeof(icpmi_gate_info) == 16", "sizeof(icpmi_stream_info) == 24", "sizeof(icpmi_robust) == 24",
                   "sizeof(icpmi_robust_info) == 24"):
        assert pinned in text
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, src])


def test_the_header_is_plain_c_and_declares_the_entry_points():
    probe = ('#include "icp_mi355x.h"\n'
             'int main(void) {\n'
             '    icpmi_robust r = {ICPMI_ROBUST_HUBER, 0, 0.1, 2.0}; icpmi_robust_info i = {0.0, 0, 0};\n'
             '    int (*a)(icpmi_ctx *, const double *, int64_t, const double *, int64_t, const icpmi_config *, const icpmi_robust *,\n'
             '             icpmi_result *, icpmi_robust_info *, double *, int32_t) = icpmi_align_robust;\n'
             '    int (*b)(icpmi_ctx *, const double *, int64_t, const double *, int64_t, const icpmi_config *, const icpmi_robust *,\n'
             '             icpmi_result *, icpmi_robust_info *, double *, int32_t) = icpmi_align_robust_device;\n'
             '    int (*c)(icpmi_ctx *, int32_t, const double *const *, const int64_t *, const double *const *, const int64_t *,\n'
             '             const icpmi_config *, const icpmi_robust *, icpmi_result *, icpmi_robust_info *, double *, int32_t,\n'
             '             int32_t *) = icpmi_align_robust_batch;\n'
             '    int (*d)(icpmi_loop *, int32_t, double) = icpmi_loop_set_robust;\n'
             '    int (*e)(const icpmi_loop *, double *, int64_t, int64_t *) = icpmi_loop_last_weights;\n'
             '    int (*f)(icpmi_ctx *, const icpmi_robust *) = icpmi_stream_set_robust;\n'
             '    int (*g)(icpmi_ctx *, icpmi_robust_info *) = icpmi_stream_last_robust;\n'
             '    return (int)(r.scale + (double)i.pairs) * 0 + (a && b && c && d && e && f && g ? 0 : 1) + ICPMI_ROBUST_GEMAN_MCCLURE - 2;\n'
             '}\n')
    subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-x", "c", "-"],
                   input=probe, text=True, check=True)


def test_the_contract_is_in_the_header_and_in_the_kernels_header():
    for path in (os.path.join(INCLUDE, "icp_mi355x.h"),
                 os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc", "icp_robust.h")):
        text = re.sub(r"\s+", "", open(path).read())
        for words in ("w=a<=k?1.0:k/a", "t=s+b*b", "r=s/t", "w=r*r", "DBL_MAX"):
            assert words in text, (path, words)


def test_ctypes_mirrors_agree():
    from lidar_slam_from_scratch_amd import capi
    assert C.sizeof(capi.Config) == 152 and C.sizeof(capi.Result) == 152
    assert C.sizeof(capi.Gate) == 16 and C.sizeof(capi.GateInfo) == 16 and C.sizeof(capi.StreamInfo) == 24
    assert C.sizeof(capi.Robust) == 24 and C.sizeof(capi.RobustInfo) == 24
    assert (capi.Robust.kind.offset, capi.Robust.scale.offset, capi.Robust.max_distance.offset) == (0, 8, 16)
    assert (capi.RobustInfo.weight_sum.offset, capi.RobustInfo.pairs.offset, capi.RobustInfo.rows.offset) == (0, 8, 16)
    assert (capi.ROBUST_HUBER, capi.ROBUST_GEMAN_MCCLURE) == (1, 2)
    for name in ("icpmi_align_robust", "icpmi_align_robust_device", "icpmi_align_robust_batch", "icpmi_loop_set_robust",
                 "icpmi_loop_last_weights", "icpmi_stream_set_robust", "icpmi_stream_last_robust"):
        assert name in capi.EXPORTS
    r = capi.as_robust((capi.ROBUST_GEMAN_MCCLURE, 0.3, 2.0))
    assert (r.kind, r.scale, r.max_distance) == (2, 0.3, 2.0) and capi.as_robust(r) is r
    assert capi.as_robust((1, 0.1)).max_distance == 0.0
