// icp_robust.h -- robust row weights (icpmi_align_robust*).
//
// Per pass, for row i with nearest target j (`found` as in k_reduce_gated), in unfused fp64 and in this order:
//     e  = q_j - p_i
//     d2 = (e0 * e0 + e1 * e1) + e2 * e2
//     b  = (e0 * n0 + e1 * n1) + e2 * n2          (icp.hpp:116)
// Gate: the row is kept iff found && d2 <= g2, with g2 = max_distance * max_distance when a gate is given and DBL_MAX
// when max_distance == 0 (a NaN or infinite row is then still dropped).
// Weight of a kept row, a = fabs(b):
//     Huber           w = a <= k ? 1.0 : k / a
//     Geman-McClure   s = k * k (formed on the host, once),  t = s + b * b,  r = s / t,  w = r * r
// Sums over the kept rows, wJ[r] = w * J[r]: columns 0..20 add wJ[r] * J[c], columns 21..26 add wJ[r] * b, column 27 adds
// (w * b) * b, column 28 adds w, column 29 adds 1.0 (the pairs); the loops and the order of additions are k_reduce_gated's
// and a dropped row adds nothing.  With w == 1.0 every product is the unweighted one: a Huber scale above every |b| gives
// the gated call's bits, and with no gate icpmi_align's.
// error = sqrt(sums[27] / sums[28]), the weighted RMS; the no-pairs rule is icp_gated.h's on !(sums[28] > 0).
//
//   k_reduce_robust        k_reduce_gated with the weight; 30 columns in the partial row (kSumsStride stays 32); the
//                          instantiation k_reduce_rule<RuleRobust, double, int, double> (kernels.h)
//   k_finish_step_robust   k_finish_step_gated over 30 columns: weight sum and pairs are fixed-order sums of columns 28, 29
//   k_icp_small_robust     icp_small_kernel.inc's third expansion: the weight on the winner that step 4 already holds
#pragma once
#include "kernels.h"

namespace icpmi {

constexpr int kRobustHuber = 1;        // ICPMI_ROBUST_HUBER
constexpr int kRobustGemanMcClure = 2; // ICPMI_ROBUST_GEMAN_MCCLURE
constexpr int kNumRobustSums = 30;     // 28 weighted sums + the weight sum + the pairs
static_assert(kNumRobustSums <= kSumsStride, "a partial row holds the robust columns");

// `kind` is a kernel argument, uniform across the wave; ks = k for Huber, k * k for Geman-McClure.  One fp64 division.
__device__ __forceinline__ double robust_weight(const int kind, const double ks, const double b)
{
    if (kind == kRobustHuber) {
        const double a = fabs(b);
        return a <= ks ? 1.0 : ks / a;
    }
    const double t = ks + b * b;
    const double r = ks / t;
    return r * r;
}

} // namespace icpmi

#include "icp_gated.h" // (icp_small.h's constants and helpers, step_no_pairs)

namespace icpmi {

#define ICPMI_SMALL_GATED 1
#define ICPMI_SMALL_ROBUST 1
#include "icp_small_kernel.inc"
#undef ICPMI_SMALL_ROBUST
#undef ICPMI_SMALL_GATED

// the weights as a rule of the k_reduce / k_finish_step families (kernels.h, RuleNone)
struct RuleRobust {
    static constexpr bool kCounted = true, kWeighted = true;
    static constexpr int kCols = kNumRobustSums;
    double g2;
    int kind;
    double ks;
    __device__ __forceinline__ double weight(const double b) const { return robust_weight(kind, ks, b); }
};

__global__ __launch_bounds__(kFinishThreads) void k_finish_step_robust(const double *__restrict__ partials,
                                                                        int nblocks, IcpState *st,
                                                                        double *history, int final_pass, int *progress,
                                                                        int ticket)
{
    finish_step_rows<RuleRobust>(partials, nblocks, 0, st, history, final_pass, progress, ticket);
}

} // namespace icpmi
