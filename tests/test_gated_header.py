"""The gate's C++ mirror compiles clean from a plain C++17 program, and the C ABI's existing structs keep their layout:
tests/cpp/gated_demo.cpp holds sizeof / offsetof static assertions on icpmi_config and icpmi_result with the values they
had before the gate existed, and the ctypes mirrors agree."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gated_demo_is_clean_cpp17_and_the_structs_keep_their_layout():
    src = os.path.join(ROOT, "tests", "cpp", "gated_demo.cpp")
    text = open(src).read()
    assert "sizeof(icpmi_config) == 152" in text and "sizeof(icpmi_result) == 152" in text
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "include"), src])


def test_the_header_is_plain_c():
    probe = '#include "icp_mi355x.h"\nint main(void) { icpmi_gate g = {2.0, {0, 0}}; icpmi_gate_info i = {0, 0}; return (int)(g.max_distance + i.pairs) * 0; }\n'
    subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-x", "c", "-"], input=probe, text=True, check=True)


def test_ctypes_mirrors_agree():
    from lidar_slam_from_scratch_amd import capi
    assert C.sizeof(capi.Config) == 152 and C.sizeof(capi.Result) == 152
    assert C.sizeof(capi.Gate) == 16 and C.sizeof(capi.GateInfo) == 16
    assert capi.Config.initial_transform.offset == 24 and capi.Result.final_error.offset == 136
    for name in ("icpmi_align_gated", "icpmi_align_gated_device", "icpmi_align_gated_batch", "icpmi_loop_set_gate"):
        assert name in capi.EXPORTS
