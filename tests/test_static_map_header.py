"""The static map off the device: the C++ mirror's demo compiles clean; the C header is plain C, its new
structs have the layout the ctypes mirrors assume and no existing struct moved; and the contract stands in the same words
in the C header, the kernels' header and the CPU restatement."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def test_static_map_demo_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE,
                           os.path.join(ROOT, "tests", "cpp", "static_map_demo.cpp")])


def test_the_header_is_plain_c_and_no_struct_moved():
    probe = ('#include <stddef.h>\n#include "icp_mi355x.h"\n'
             '_Static_assert(sizeof(icpmi_static_rule) == 16 && offsetof(icpmi_static_rule, min_probability) == 0\n'
             '               && offsetof(icpmi_static_rule, min_observations) == 4 && offsetof(icpmi_static_rule, reserved) == 8,\n'
             '               "icpmi_static_rule");\n'
             '_Static_assert(sizeof(icpmi_static_info) == 120 && offsetof(icpmi_static_info, rows) == 0 && offsetof(icpmi_static_info, voting) == 8\n'
             '               && offsetof(icpmi_static_info, dropped) == 16 && offsetof(icpmi_static_info, kept) == 24\n'
             '               && offsetof(icpmi_static_info, live) == 32, "icpmi_static_info");\n'
             '_Static_assert(sizeof(icpmi_grid_config) == 32 && offsetof(icpmi_grid_config, max_range) == 24, "icpmi_grid_config");\n'
             '_Static_assert(sizeof(icpmi_raster_info) == 40 && offsetof(icpmi_raster_info, n_free) == 32, "icpmi_raster_info");\n'
             '_Static_assert(sizeof(icpmi_counts_info) == 56 && offsetof(icpmi_counts_info, resolution) == 16\n'
             '               && offsetof(icpmi_counts_info, n_hit_cells) == 32 && offsetof(icpmi_counts_info, frames_used) == 48,\n'
             '               "icpmi_counts_info");\n'
             '_Static_assert(sizeof(icpmi_live_info) == 88 && offsetof(icpmi_live_info, frames_cast) == 56 && offsetof(icpmi_live_info, rebuilt) == 64\n'
             '               && offsetof(icpmi_live_info, moved) == 68 && offsetof(icpmi_live_info, plane_x0) == 72\n'
             '               && offsetof(icpmi_live_info, plane_h) == 84, "icpmi_live_info");\n'
             '_Static_assert(sizeof(icpmi_ground_config) == 72 && sizeof(icpmi_ground_info) == 32, "the ground structs");\n'
             '_Static_assert(sizeof(icpmi_config) == 152 && sizeof(icpmi_result) == 152 && sizeof(icpmi_gate) == 16\n'
             '               && sizeof(icpmi_gate_info) == 16 && sizeof(icpmi_robust) == 24 && sizeof(icpmi_robust_info) == 24\n'
             '               && sizeof(icpmi_stream_info) == 24 && sizeof(icpmi_normal_matrix) == 488 && sizeof(icpmi_gicp) == 24\n'
             '               && sizeof(icpmi_gicp_info) == 16 && sizeof(icpmi_deskew_config) == 104 && sizeof(icpmi_options) == 16,\n'
             '               "the other structs");\n'
             'int main(void) {\n'
             '    icpmi_static_rule r = {ICPMI_STATIC_MIN_PROBABILITY_DEFAULT, ICPMI_STATIC_MIN_OBSERVATIONS_DEFAULT, 0};\n'
             '    int (*a)(icpmi_map *, const double *, int64_t, const icpmi_grid_config *, const icpmi_static_rule *, int64_t, double *,\n'
             '             int64_t, int64_t *, icpmi_static_info *) = icpmi_map_world_static;\n'
             '    int (*b)(icpmi_map *, const double *, int64_t, const icpmi_grid_config *, const icpmi_static_rule *, double, double *,\n'
             '             int64_t, int64_t *, icpmi_static_info *) = icpmi_map_finish_static;\n'
             '    int (*c)(icpmi_map *, int64_t, uint8_t *, int64_t, int64_t *) = icpmi_map_static_labels;\n'
             '    return (r.min_probability == 50 && r.min_observations == 3 && a && b && c) ? 0 : 1;\n'
             '}\n')
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-x", "c", "-"],
                   input=probe, text=True, check=True)


def test_ctypes_mirrors_agree():
    from lidar_slam_from_scratch_amd import capi
    import static_map_ref as ref
    assert C.sizeof(capi.StaticRule) == 16 and C.sizeof(capi.StaticInfo) == 120 and C.sizeof(capi.LiveInfo) == 88
    assert (capi.StaticRule.min_probability.offset, capi.StaticRule.min_observations.offset, capi.StaticRule.reserved.offset) == (0, 4, 8)
    assert (capi.StaticInfo.rows.offset, capi.StaticInfo.voting.offset, capi.StaticInfo.dropped.offset, capi.StaticInfo.kept.offset,
            capi.StaticInfo.live.offset) == (0, 8, 16, 24, 32)
    r = capi.StaticRule()
    assert (r.min_probability, r.min_observations, r.reserved) == (50, 3, 0) == (ref.MIN_PROBABILITY_DEFAULT, ref.MIN_OBSERVATIONS_DEFAULT, 0)
    assert (capi.STATIC_MIN_PROBABILITY_DEFAULT, capi.STATIC_MIN_OBSERVATIONS_DEFAULT) == (50, 3)
    assert (capi.STATIC_QUIET, capi.STATIC_VOTES, capi.STATIC_DROPPED) == (ref.QUIET, ref.VOTES, ref.DROPPED) == (0, 1, 2)
    g = capi.as_static_rule((30, 5))
    assert (g.min_probability, g.min_observations, g.reserved) == (30, 5, 0) and capi.as_static_rule(g) is g
    for name in ("icpmi_map_world_static", "icpmi_map_finish_static", "icpmi_map_static_labels"):
        assert name in capi.EXPORTS


def _contract(path, first, last):
    """the contract's lines of a file, comment marks and indentation stripped"""
    lines = open(path).read().splitlines()
    strip = [re.sub(r"^\s*(//|\*|/\*)?\s*", "", ln).rstrip() for ln in lines]
    a = next(k for k, ln in enumerate(strip) if ln.startswith(first))
    b = next(k for k, ln in enumerate(strip) if k > a and ln.startswith(last))
    return [ln for ln in strip[a:b + 1] if ln]


def test_the_contract_is_stated_in_the_same_words_three_times():
    first, last = "A row of used frame i VOTES iff", "nothing.  All integer:"
    paths = (os.path.join(INCLUDE, "icp_mi355x.h"), os.path.join(CSRC, "static_map.h"), os.path.join(ROOT, "scripts", "static_map_ref.py"))
    texts = [_contract(p, first, last) for p in paths]
    assert len(texts[0]) == 9
    assert texts[0] == texts[1] == texts[2]
    for path in paths:
        text = open(path).read()
        assert "raycast_counts" in text and "min_observations" in text
    # the header says which rows can vote at all under the default band
    header = open(paths[0]).read()
    assert "never votes" in header and "icpmi_map_set_ground" in header
