// icp_gated.h -- the correspondence-distance gate (icpmi_align_gated*).
//
// With g2 = max_distance * max_distance (fp64, formed once on the host) a pass keeps row i with nearest target j iff
//     e = q_j - p_i;   d2 = (e0 * e0 + e1 * e1) + e2 * e2   (unfused, this order);   d2 <= g2
// A row with a non-finite coordinate, or without a neighbour, is dropped (the comparison is false for a NaN).  The 28
// sums run over the kept rows, column 28 of every partial row is its block's number of kept rows, and the step divides
// by their sum: error = sqrt(sum b^2 / kept).  A pass that keeps no row ends the loop without convergence.
//
//   k_reduce_gated        k_reduce (kernels.h) with the test: same grid, same order of additions, so a gate that keeps
//                         every row leaves k_reduce's bits in columns 0..27
//   k_finish_step_gated   k_finish_step with the count taken from column 28 and the no-pairs rule in front of the step
//   k_icp_small_gated     icp_small.h: the small-cloud kernel's body with the test on the winner it already holds
#pragma once
#include "icp_small.h"
#include "kernels.h"

namespace icpmi {

__global__ __launch_bounds__(256) void k_reduce_gated(const double *__restrict__ cur, int n,
                                                      const double *__restrict__ tgt, int m_tgt,
                                                      const double *__restrict__ nrm,
                                                      const int *__restrict__ idx,
                                                      double *__restrict__ partials,
                                                      const IcpState *__restrict__ st, const double g2)
{
    if (st && st->done) return;
    double acc[28];
#pragma unroll
    for (int e = 0; e < 28; ++e) acc[e] = 0.0;
    double kept = 0.0; // (a small integer: exact in any order of additions)
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int ji = idx ? idx[i] : i;
        const bool found = (unsigned)ji < (unsigned)m_tgt; // (-1: a non-finite row has no neighbour, kdtree.hpp:53)
        const int j = found ? ji : 0;                      // the gather stays in bounds
        const double p0 = cur[3 * i], p1 = cur[3 * i + 1], p2 = cur[3 * i + 2];
        const double q0 = tgt[3 * j], q1 = tgt[3 * j + 1], q2 = tgt[3 * j + 2];
        const double n0 = nrm[3 * j], n1 = nrm[3 * j + 1], n2 = nrm[3 * j + 2];
        const double d0 = q0 - p0, d1 = q1 - p1, d2 = q2 - p2;
        if (!(found && (d0 * d0 + d1 * d1) + d2 * d2 <= g2)) continue; // gated out: nothing is added, not even a zero
        double J[6];
        J[0] = p1 * n2 - p2 * n1; // p x n, icp.hpp:105
        J[1] = p2 * n0 - p0 * n2;
        J[2] = p0 * n1 - p1 * n0;
        J[3] = n0;
        J[4] = n1;
        J[5] = n2;
        const double b = (d0 * n0 + d1 * n1) + d2 * n2; // icp.hpp:116
        int o = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) acc[o++] += J[r] * J[c];
#pragma unroll
        for (int r = 0; r < 6; ++r) acc[21 + r] += J[r] * b;
        acc[27] += b * b;
        kept += 1.0;
    }
    __shared__ double red[4][29];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < 28; ++e) {
        const double s = wave_sum(acc[e]);
        if (lane == 0) red[wave][e] = s;
    }
    {
        const double s = wave_sum(kept);
        if (lane == 0) red[wave][28] = s;
    }
    __syncthreads();
    if (threadIdx.x < 29) {
        const int e = threadIdx.x;
        partials[(size_t)blockIdx.x * kSumsStride + e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
    }
}

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
    __shared__ IcpState ls, sums; // `sums`: only its sums[] are used
    state_copy(&ls, st);
    finish_sums<true>(partials, nblocks, 0, &sums);
    __syncthreads();
    if (!ls.done && threadIdx.x < kNumSums) ls.sums[threadIdx.x] = sums.sums[threadIdx.x];
    __syncthreads();
    if (threadIdx.x < 64) {
        const bool none = !ls.done && !(ls.sums[28] > 0.0); // wave-uniform
        __builtin_amdgcn_wave_barrier();
        if (none) {
            if (threadIdx.x == 0) step_no_pairs(&ls, history, final_pass);
        } else {
            step_update_wave(&ls, history, final_pass, threadIdx.x);
        }
        if (threadIdx.x == 0) publish_progress(progress, ticket, ls.done);
    }
    __syncthreads();
    state_copy(st, &ls);
}

} // namespace icpmi
