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
//   k_reduce_robust        k_reduce_gated with the weight; 30 columns in the partial row (kSumsStride stays 32)
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

__global__ __launch_bounds__(256) void k_reduce_robust(const double *__restrict__ cur, int n,
                                                       const double *__restrict__ tgt, int m_tgt,
                                                       const double *__restrict__ nrm,
                                                       const int *__restrict__ idx,
                                                       double *__restrict__ partials,
                                                       const IcpState *__restrict__ st, const double g2,
                                                       const int kind, const double ks)
{
    if (st && st->done) return;
    double acc[28];
#pragma unroll
    for (int e = 0; e < 28; ++e) acc[e] = 0.0;
    double wsum = 0.0;
    double kept = 0.0; // (a small integer: exact in any order of additions)
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int ji = idx ? idx[i] : i;
        const bool found = (unsigned)ji < (unsigned)m_tgt; // (-1: a non-finite row has no neighbour, kdtree.hpp:53)
        const int j = found ? ji : 0;                      // the gather stays in bounds
        const double p0 = cur[3 * i], p1 = cur[3 * i + 1], p2 = cur[3 * i + 2];
        const double q0 = tgt[3 * j], q1 = tgt[3 * j + 1], q2 = tgt[3 * j + 2];
        const double n0 = nrm[3 * j], n1 = nrm[3 * j + 1], n2 = nrm[3 * j + 2];
        const double d0 = q0 - p0, d1 = q1 - p1, d2 = q2 - p2;
        if (!(found && (d0 * d0 + d1 * d1) + d2 * d2 <= g2)) continue; // dropped: nothing is added, not even a zero
        double J[6];
        J[0] = p1 * n2 - p2 * n1; // p x n, icp.hpp:105
        J[1] = p2 * n0 - p0 * n2;
        J[2] = p0 * n1 - p1 * n0;
        J[3] = n0;
        J[4] = n1;
        J[5] = n2;
        const double b = (d0 * n0 + d1 * n1) + d2 * n2; // icp.hpp:116
        const double w = robust_weight(kind, ks, b);
        double wJ[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) wJ[r] = w * J[r];
        int o = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) acc[o++] += wJ[r] * J[c];
#pragma unroll
        for (int r = 0; r < 6; ++r) acc[21 + r] += wJ[r] * b;
        acc[27] += (w * b) * b;
        wsum += w;
        kept += 1.0;
    }
    __shared__ double red[4][kNumRobustSums];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < 28; ++e) {
        const double s = wave_sum(acc[e]);
        if (lane == 0) red[wave][e] = s;
    }
    {
        const double s = wave_sum(wsum), c = wave_sum(kept);
        if (lane == 0) red[wave][28] = s, red[wave][29] = c;
    }
    __syncthreads();
    if (threadIdx.x < kNumRobustSums) {
        const int e = threadIdx.x;
        partials[(size_t)blockIdx.x * kSumsStride + e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
    }
}

__global__ __launch_bounds__(kFinishThreads) void k_finish_step_robust(const double *__restrict__ partials,
                                                                        int nblocks, IcpState *st,
                                                                        double *history, int final_pass, int *progress,
                                                                        int ticket)
{
    __shared__ IcpState ls, sums; // `sums`: only its sums[] are used
    state_copy(&ls, st);
    finish_sums<true, kNumRobustSums>(partials, nblocks, 0, &sums);
    __syncthreads();
    if (!ls.done && threadIdx.x < kNumRobustSums) ls.sums[threadIdx.x] = sums.sums[threadIdx.x];
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
