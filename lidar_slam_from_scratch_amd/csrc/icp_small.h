// icp_small.h -- one ICP iteration's search + residual work for SMALL clouds in ONE kernel.
//
// The reference's real caller registers voxel-filtered scans of 5-20k points against each other
// (slam_node.cpp:134-138, loop_closure.hpp:105-109): the target is a handful of 2048-target splits.
// There the general path -- k_nn_coarse (minima of every (query, split) to memory), k_nn_resolve4
// (reads them back, exact scans, normal-equation terms) and the pose update of the points -- is
// three dependent launches of a few microseconds each for ~2 us of matrix work, and the
// intermediate is written and read again for nothing.  k_icp_small does an iteration's row work
// in one launch and keeps the intermediate in LDS.  (Measured with in-kernel clocks and dropped:
// four waves per workgroup with whole splits per wave -- fewer instructions in all, but one wave per
// SIMD leaves every MFMA -> minimum dependency and every load exposed: 30k cycles against 21k; slot
// scans by the whole wave with DPP reductions instead of quarter-waves: 6.4k cycles against 4.4k; the step of
// the PREVIOUS pass -- k_finish_step's work -- repeated by every workgroup at the head of this kernel, so that
// an iteration is one launch: 21.0 us per iteration against 20.3, the serial step does not hide under the
// operand stream but in front of an issue-bound remainder, and 250 workgroups sitting through it keep a
// second stream's kernels off the chip: 0.37 ms per frame of the file stream against 0.32.)
//
//   workgroup = 32 rows (one MFMA tile of queries) x ALL splits, 8 waves = two per SIMD.
//   1. every wave loads the 32 rows and moves them by the pending pose update (icp.hpp:174-176
//      for the first pass, :225-226 afterwards; same operation order as k_transform), wave 0
//      stores the moved rows;
//   2. the target's half-splits (32 tiles = 1024 targets) are dealt to the waves; a wave builds its
//      A operands about the split's centre (coarse_build_a's arithmetic), streams its 32 B tiles
//      from memory straight into registers (no other wave wants them: no LDS staging, no
//      workgroup barrier) and runs the coarse loop and the 1-NN epilogue of nn_mfma.h: the
//      (column-tagged minimum, second minimum) of every row against its half-split -> LDS;
//   3. the resolve of nn_mfma.h on those records, one row per quarter-wave as k_nn_resolve4:
//      per-split records merged from the two halves, smallest split, exact fp64 scan of the
//      winning slot, certificate (split_tau; slots / whole splits under the bound rescanned).  The scan also fetches each
//      candidate's NORMAL from a Morton-ordered copy, so the winner's matched point and normal
//      are at hand when it is known: no dependent gather;
//   4. J row and b of every row (icp.hpp:99-117), summed per workgroup in k_nn_resolve4<8>'s
//      order: the partial rows -- hence error history and pose -- are bit-identical to the general
//      path's (tests/test_gpu_parity.py::test_small_cloud_kernel_gives_the_general_path_bits).
//
// The certificate argument is nn_mfma.h's: the records are exactly the values k_nn_coarse would have
// written (same operands, same MFMA, same epilogue; the second minimum kept in fp32 instead of
// bf16 rounded down, which only tightens it), so the result is the exact fp64 nearest neighbour,
// ties to the lowest original index.
#pragma once
#include "nn_mfma.h"

namespace icpmi {

constexpr int kSmallWaves = 8;
constexpr int kSmallThreads = 64 * kSmallWaves;
// (kSmallQ = 32 rows (queries) per workgroup: loop_plan.h)
constexpr int kSmallUnitTiles = 32;                          // target tiles per unit of a wave's work
constexpr int kSmallUnitsPerSplit = kSplitTiles / kSmallUnitTiles;
constexpr int kSmallMaxSplits = 16;                          // one lane of a quarter-wave per split
static_assert(kSmallQ == 4 * kSmallWaves, "one row per quarter-wave in the resolve part");
static_assert(kSplitTiles % kSmallUnitTiles == 0 && kSmallUnitTiles % 2 == 0, "whole units, tiles in pairs");
static_assert(kSlotTargets == 64, "the slot scan takes four targets per lane of a quarter-wave");

// (v1, v2) <- the two smallest column minima of the union of two records over the SAME columns
// (two halves of a split).  If both minima sit in the same column the other half's minimum is not
// a second column.
__device__ __forceinline__ void small_merge(float &v1, float &v2, const float w1, const float w2)
{
    const bool same = ((__float_as_uint(v1) ^ __float_as_uint(w1)) & 31u) == 0u;
    const float lo = w1 < v1 ? w1 : v1, hi = w1 < v1 ? v1 : w1;
    float n2 = w2 < v2 ? w2 : v2;
    if (!same) n2 = hi < n2 ? hi : n2;
    v1 = lo;
    v2 = n2;
}

// The kernel's text is in icp_small_kernel.inc, compiled twice: k_icp_small, and k_icp_small_gated with the
// correspondence-distance gate of icp_gated.h.  Shared as text, not as a `template <bool Gated>` body inlined into two
// __global__ wrappers: inlined, k_icp_small keeps its resource line but not its instructions (197 lines of its ISA
// differ: registers renamed, loads moved), and the ungated kernel must stay the kernel that was measured.
// (A third expansion, k_icp_small_robust with ICPMI_SMALL_ROBUST 1, is icp_robust.h's.)
#define ICPMI_SMALL_ROBUST 0
#define ICPMI_SMALL_GATED 0
#include "icp_small_kernel.inc"
#undef ICPMI_SMALL_GATED
#define ICPMI_SMALL_GATED 1
#include "icp_small_kernel.inc"
#undef ICPMI_SMALL_GATED
#undef ICPMI_SMALL_ROBUST

} // namespace icpmi
