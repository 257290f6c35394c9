// icp_gated.h -- the correspondence-distance gate (icpmi_align_gated*).
//
// With g2 = max_distance * max_distance (fp64, formed once on the host) a pass keeps row i with nearest target j iff
//     e = q_j - p_i;   d2 = (e0 * e0 + e1 * e1) + e2 * e2   (unfused, this order);   d2 <= g2
// A row with a non-finite coordinate, or without a neighbour, is dropped (the comparison is false for a NaN).  The 28
// sums run over the kept rows, column 28 of every partial row is its block's number of kept rows, and the step divides
// by their sum: error = sqrt(sum b^2 / kept).  A pass that keeps no row ends the loop without convergence.
//
//   k_reduce_gated        k_reduce (kernels.h) with the test: same grid, same order of additions, so a gate that keeps
//                         every row leaves k_reduce's bits in columns 0..27; the instantiation k_reduce_rule<RuleGate, double>
//   k_finish_step_gated   k_finish_step with the count taken from column 28 and the no-pairs rule in front of the step
//   k_icp_small_gated     icp_small.h: the small-cloud kernel's body with the test on the winner it already holds
#pragma once
#include "icp_small.h"
#include "kernels.h"

namespace icpmi {

// the gate as a rule of the k_reduce / k_finish_step families (kernels.h, RuleNone)
struct RuleGate {
    static constexpr bool kCounted = true, kWeighted = false;
    static constexpr int kCols = 29;
    double g2;
};

// A pass that kept no row, by the first wave's lane 0: the loop is left as by a break, without convergence -- +Inf is that
// pass's error and, entered at once like a convergence break's (step_update), the post-loop entry.  A post-loop pass
// (after exhaustion) that keeps no row enters +Inf once.  The pose is what had accumulated.
__device__ inline void step_no_pairs(IcpState *st, double *history, int final_pass)
{
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const int hist_len = st->hist_len, max_hist = st->max_hist;
    if (history && hist_len < max_hist) history[hist_len] = inf;
    st->last_error = inf;
    st->final_error = inf;
    st->done = 1;
    if (final_pass) {
        st->hist_len = hist_len + 1;
        return;
    }
    st->loops += 1;
    if (history && hist_len + 1 < max_hist) history[hist_len + 1] = inf;
    st->hist_len = hist_len + 2;
    st->finalized = 1;
}

__global__ __launch_bounds__(kFinishThreads) void k_finish_step_gated(const double *__restrict__ partials,
                                                                       int nblocks, IcpState *st,
                                                                       double *history, int final_pass, int *progress,
                                                                       int ticket)
{
    finish_step_rows<RuleGate>(partials, nblocks, 0, st, history, final_pass, progress, ticket);
}

} // namespace icpmi
