"""The small form of plane-to-plane ICP off the device (addendum): the plan's new fact -- with it a
plane-to-plane call is small exactly where a gated call is, with the gated call's partial rows, and without it the plan is
what it was; the C ABI's new words compile as plain C and leave icpmi_gicp's layout alone; the C++ and ctypes mirrors."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc")


def test_the_plan_of_a_small_form_call(tmp_path):
    probe = ('#include <cstdio>\n#include <cstring>\n#include "loop_plan.h"\nusing namespace icpmi;\n'
             'int main() {\n'
             '    int bad = 0, small = 0;\n'
             '    const int engines[] = {ICPMI_SEARCH_EXACT_F64, ICPMI_SEARCH_MFMA_BF16};\n'
             '    for (int engine : engines) for (int pruned = 0; pruned < 2; ++pruned) for (int comm = 0; comm < 2; ++comm)\n'
             '    for (int n : {0, 1, 5, 33, 1001, 8799, 32736, 32737, 32768, 32769, 65537, 1000000}) for (int splits : {1, 3, 8, 9, 13, 49, 500}) {\n'
             '        LoopFacts f; f.n = n; f.m = splits * 2048; f.nn_engine = engine; f.nn_pruned = pruned && engine == ICPMI_SEARCH_MFMA_BF16;\n'
             '        f.nn_splits = splits; f.comm = comm != 0; f.rule = kRuleGicp;\n'
             '        const LoopPlan general = make_loop_plan(f);\n'
             '        f.gicp_small = true;\n'
             '        const LoopPlan p = make_loop_plan(f);\n'
             '        LoopFacts g = f; g.rule = kRuleGate; g.gicp_small = false;\n'
             '        const LoopPlan q = make_loop_plan(g);\n'
             '        LoopFacts h = g; h.gicp_small = true;                  // the fact is the plane-to-plane rule\'s alone\n'
             '        const LoopPlan q2 = make_loop_plan(h);\n'
             '        bool ok = p.rule == kRuleGicp && !p.error && p.small == q.small && !p.fused && !p.pruned && !p.bounded && !p.reuse &&\n'
             '            !p.fused_tail && !p.cull_full && !p.sort_source && !general.small && !general.error &&\n'
             '            q2.small == q.small && q2.rblocks == q.rblocks && q2.fin_blocks == q.fin_blocks && !q2.error;\n'
             '        if (p.small) ok = ok && p.rblocks == (n + kSmallQ - 1) / kSmallQ && p.rblocks == q.rblocks && !comm && n <= kSmallMaxQueries &&\n'
             '            splits <= kSmallSplitsDefault && engine == ICPMI_SEARCH_MFMA_BF16;\n'
             '        else ok = ok && p.rblocks == general.rblocks && p.fin_blocks == general.fin_blocks && p.sum_tree == general.sum_tree;\n'
             '        small += p.small;\n'
             '        if (!ok) { std::printf("n %d splits %d engine %d pruned %d comm %d\\n", n, splits, engine, pruned, comm); ++bad; }\n'
             '    }\n'
             '    return bad || !small ? 1 : 0;\n'
             '}\n')
    exe = str(tmp_path / "gicp_small_plan_probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-x", "c++", "-", "-o", exe],
                   input=probe, text=True, check=True)
    subprocess.check_call([exe])


def test_the_header_is_plain_c_and_the_layout_stands():
    probe = ('#include <stddef.h>\n#include "icp_mi355x.h"\n'
             '_Static_assert(sizeof(icpmi_gicp) == 24 && offsetof(icpmi_gicp, epsilon) == 0 && offsetof(icpmi_gicp, max_distance) == 8\n'
             '               && offsetof(icpmi_gicp, reserved) == 16 && ICPMI_GICP_FORM_SMALL == 1, "icpmi_gicp");\n'
             'int main(void) {\n'
             '    icpmi_gicp r = {ICPMI_GICP_EPSILON_DEFAULT, 2.0, ICPMI_GICP_FORM_SMALL};\n'
             '    int (*a)(icpmi_ctx *, int32_t, const double *const *, const int64_t *, const double *const *, const int64_t *,\n'
             '             const icpmi_config *, const icpmi_gicp *, icpmi_result *, icpmi_gicp_info *, double *, int32_t, int32_t *) =\n'
             '        icpmi_align_gicp_batch;\n'
             '    int (*b)(icpmi_loop *, double) = icpmi_loop_set_gicp;\n'
             '    return (int)r.reserved * 0 + (a && b ? 0 : 1);\n'
             '}\n')
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-x", "c", "-"],
                   input=probe, text=True, check=True)


def test_the_cpp_mirror_is_clean_cpp17():
    for name in ("gicp_loop_demo.cpp",):
        subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE,
                        os.path.join(ROOT, "tests", "cpp", name)], check=True)
    probe = ('#include "icp_mi355x.hpp"\n'
             'int main() {\n'
             '    icp_mi355x::GicpRule rule;\n'
             '    icp_mi355x::LoopClosureConfig cfg;\n'
             '    return !rule.small_form && cfg.gicp_epsilon == 0.0 && &icp_mi355x::align_gicp_batch ? 0 : 1;\n'
             '}\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-address", "-I", INCLUDE, "-x", "c++", "-"],
                   input=probe, text=True, check=True)


def test_ctypes_mirrors_agree():
    from lidar_slam_from_scratch_amd import capi
    from lidar_slam_from_scratch_amd import loop_closure as lc
    assert capi.GICP_FORM_SMALL == 1 and C.sizeof(capi.Gicp) == 24
    for name in ("icpmi_align_gicp_batch", "icpmi_loop_set_gicp"):
        assert name in capi.EXPORTS
    assert capi.as_gicp((1e-3, 2.0, True)).reserved == capi.GICP_FORM_SMALL
    assert capi.as_gicp((1e-3, 2.0, False)).reserved == 0 and capi.as_gicp((1e-3, 2.0)).reserved == 0 and capi.as_gicp((0.5,)).reserved == 0
    assert lc.LoopClosureConfig().gicp_epsilon == 0.0 and lc.LoopClosureConfig(gicp_epsilon=1e-3).gicp_epsilon == 1e-3
