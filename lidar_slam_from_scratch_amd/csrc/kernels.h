// kernels.h -- HIP kernels of the point-to-plane ICP path for gfx950 (wave64).
//
//   k_nn_f64          exact fp64 exhaustive nearest neighbour (kdtree.hpp:43-59,112-142)
//   k_nn_merge        min over target splits
//   (k-NN + PCA normals live in nn_mfma.h: k_knn_resolve / k_knn_exact_list / k_normals_from_knn)
//   k_reduce          residuals + 6x6 normal-equation partial sums (icp.hpp:99-120,198-206)
//   k_finish / k_step fixed-order final sum, error, convergence test, LDLT solve,
//                     Rodrigues, pose accumulation (icp.hpp:207-231)
//   k_transform       cloud * R^T + t^T (icp.hpp:174-176,225-226)
//   k_finish_step_transform / k_step_transform
//                     the loop's fused forms: final sum + step + pose update of the rows in one
//                     launch (single GPU) / step + pose update behind the all-reduce (sharded)
//
// All arithmetic that decides an index or a flag is fp64 in the reference's operation
// order (no FMA contraction in this TU).  Reductions use wave shuffles + LDS and a fixed
// partial order: results are run-to-run bit-stable (no float atomics).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "device_math.h"
#include "list_reuse.h"
#include "loop_plan.h"
#include "workspace_layout.h"

namespace icpmi {

constexpr int kWave = 64;
constexpr int kNumSums = 29;       // 21 JtJ (upper, row by row) + 6 Jtb + sum b^2 + count
// (kSumsStride = 32, the doubles a partial row is stored in: workspace_layout.h)
// Sharded runs all-reduce one more word: sums[kDoneSlot] = 1 on a rank whose loop has ended.
// Small integers add exactly in any order, so every rank reads the same count whatever the
// collective's algorithm: the hosts stop queueing iterations on that agreed count alone.
constexpr int kDoneSlot = 29;
constexpr int kNumExchanged = 30;

struct IcpState {
    double total[16];       // accumulated source->target transform (icp.hpp:178,229)
    double delta[16];       // last update (icp.hpp:220)
    double sums[kSumsStride];
    double prev_error;      // icp.hpp:179,231
    double last_error;
    double final_error;
    double tolerance;
    double min_error;
    int32_t hist_len;
    int32_t done;           // loop left (break or exhausted): later kernels are no-ops
    int32_t converged;
    int32_t loops;
    int32_t max_hist;
    int32_t error;          // sharded runs: the ranks disagreed on `done` (k_step)
    int32_t finalized;      // the post-loop entry (icp.hpp:235-252) is already in the history (see step_update)
    int32_t pad;
};

// ------------------------------------------------------------------------------------
// exact fp64 exhaustive 1-NN.  grid = (query blocks, target splits), 256 threads, QPT
// queries per thread held in registers.  Every lane needs the same target point at the
// same time, so targets come through the scalar unit (wave-uniform address -> s_load into
// SGPRs, broadcast to the VALU for free) instead of LDS.
// ------------------------------------------------------------------------------------
template <int QPT>
__global__ __launch_bounds__(256) void k_nn_f64(const double *__restrict__ qry, int n,
                                                const double *__restrict__ tgt, int m,
                                                int tgt_per_split,
                                                double *__restrict__ out_d2,
                                                int *__restrict__ out_idx,
                                                const IcpState *__restrict__ st)
{
    if (st && st->done) return;
    const int base = blockIdx.x * (256 * QPT) + threadIdx.x;
    double px[QPT], py[QPT], pz[QPT], best[QPT];
    int bidx[QPT];
#pragma unroll
    for (int r = 0; r < QPT; ++r) {
        const int i = base + r * 256;
        const int ic = i < n ? i : n - 1;
        px[r] = qry[3 * ic];
        py[r] = qry[3 * ic + 1];
        pz[r] = qry[3 * ic + 2];
        best[r] = 1.7976931348623157e308; // DBL_MAX, kdtree.hpp:54
        bidx[r] = -1;
    }
    const int j0 = blockIdx.y * tgt_per_split;
    const int j1 = min(m, j0 + tgt_per_split);
#pragma unroll 4
    for (int j = j0; j < j1; ++j) {
        const double tx = tgt[3 * j], ty = tgt[3 * j + 1], tz = tgt[3 * j + 2];
#pragma unroll
        for (int r = 0; r < QPT; ++r) {
            const double d = sqdist(tx, ty, tz, px[r], py[r], pz[r]);
            if (d < best[r]) { // strict: first (lowest-index) minimum wins
                best[r] = d;
                bidx[r] = j;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < QPT; ++r) {
        const int i = base + r * 256;
        if (i < n) {
            out_d2[(size_t)blockIdx.y * n + i] = best[r];
            out_idx[(size_t)blockIdx.y * n + i] = bidx[r];
        }
    }
}

// min over splits; ties -> lowest index (splits are in increasing index order)
__global__ __launch_bounds__(256) void k_nn_merge(const double *__restrict__ part_d2,
                                                  const int *__restrict__ part_idx, int n,
                                                  int splits, int *__restrict__ idx,
                                                  double *__restrict__ d2,
                                                  const IcpState *__restrict__ st)
{
    if (st && st->done) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double best = part_d2[i];
    int bi = part_idx[i];
    for (int s = 1; s < splits; ++s) {
        const double d = part_d2[(size_t)s * n + i];
        if (d < best) {
            best = d;
            bi = part_idx[(size_t)s * n + i];
        }
    }
    idx[i] = bi;
    if (d2) d2[i] = best;
}

// ------------------------------------------------------------------------------------
// residuals + normal equations.  Each thread accumulates the 28 sums over a grid-stride
// slice, then wave shuffle reduction -> LDS across the 4 waves -> one partial row per
// block.  HBM-bound gather: 24 B (p) + 4 B (idx) + 24 B (q) + 24 B (n) per point.
// When `matched` is non-null, q and n come from row i of (tgt, nrm) (icp.hpp:89-93).
// ------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

// The rule of a pass's rows (LoopRule, loop_plan.h) as the kernels of the k_reduce and k_finish_step families see it: a type
// with kCounted (the rows are tested and the kept ones counted in the partial row), kWeighted (each kept row has a weight)
// and kCols, the columns of a partial row; a counted rule carries g2, a weighted one gives weight(b).  No rule here;
// RuleGate: icp_gated.h, RuleRobust: icp_robust.h.
struct RuleNone {
    static constexpr bool kCounted = false, kWeighted = false;
    static constexpr int kCols = 28;
};

// k_reduce and its gated and robust forms: one kernel template, k_reduce_rule<RuleNone>, <RuleGate, double> and
// <RuleRobust, double, int, double> -- the rule's own arguments (g2; g2, kind, ks) follow the common ones.  Per instantiation
// the fp64 operations and their order are those of the contracts at the heads of icp_gated.h and icp_robust.h; with no
// rule every row is added (a row without a neighbour too: the sums are garbage then anyway, but the gather must stay in
// bounds).  (The body sits in the kernel itself: inlined from a device function, the compiler commuted operands.)
template <class Rule, class... RuleArgs>
__global__ __launch_bounds__(256) void k_reduce_rule(const double *__restrict__ cur, int n, const double *__restrict__ tgt, int m_tgt,
                                                     const double *__restrict__ nrm, const int *__restrict__ idx,
                                                     double *__restrict__ partials, const IcpState *__restrict__ st,
                                                     const RuleArgs... rule_args)
{
    [[maybe_unused]] const Rule rule{rule_args...};
    if (st && st->done) return;
    double acc[28];
#pragma unroll
    for (int e = 0; e < 28; ++e) acc[e] = 0.0;
    [[maybe_unused]] double wsum = 0.0;
    [[maybe_unused]] double kept = 0.0; // (a small integer: exact in any order of additions)
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int ji = idx ? idx[i] : i;
        const bool found = (unsigned)ji < (unsigned)m_tgt; // (-1: a non-finite row has no neighbour, kdtree.hpp:53)
        const int j = found ? ji : 0;                      // the gather stays in bounds
        const double p0 = cur[3 * i], p1 = cur[3 * i + 1], p2 = cur[3 * i + 2];
        const double q0 = tgt[3 * j], q1 = tgt[3 * j + 1], q2 = tgt[3 * j + 2];
        const double n0 = nrm[3 * j], n1 = nrm[3 * j + 1], n2 = nrm[3 * j + 2];
        const double d0 = q0 - p0, d1 = q1 - p1, d2 = q2 - p2;
        if constexpr (Rule::kCounted)
            if (!(found && (d0 * d0 + d1 * d1) + d2 * d2 <= rule.g2)) continue; // dropped: nothing is added, not even a zero
        double J[6];
        J[0] = p1 * n2 - p2 * n1; // p x n, icp.hpp:105
        J[1] = p2 * n0 - p0 * n2;
        J[2] = p0 * n1 - p1 * n0;
        J[3] = n0;
        J[4] = n1;
        J[5] = n2;
        const double b = (d0 * n0 + d1 * n1) + d2 * n2; // icp.hpp:116
        int o = 0;
        if constexpr (Rule::kWeighted) {
            const double w = rule.weight(b);
            double wJ[6];
#pragma unroll
            for (int r = 0; r < 6; ++r) wJ[r] = w * J[r];
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = r; c < 6; ++c) acc[o++] += wJ[r] * J[c];
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[21 + r] += wJ[r] * b;
            acc[27] += (w * b) * b;
            wsum += w;
        } else {
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = r; c < 6; ++c) acc[o++] += J[r] * J[c];
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[21 + r] += J[r] * b;
            acc[27] += b * b;
        }
        if constexpr (Rule::kCounted) kept += 1.0;
    }
    __shared__ double red[4][Rule::kCols];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < 28; ++e) {
        const double s = wave_sum(acc[e]);
        if (lane == 0) red[wave][e] = s;
    }
    if constexpr (Rule::kWeighted) {
        const double s = wave_sum(wsum), c = wave_sum(kept);
        if (lane == 0) red[wave][28] = s, red[wave][29] = c;
    } else if constexpr (Rule::kCounted) {
        const double s = wave_sum(kept);
        if (lane == 0) red[wave][28] = s;
    }
    __syncthreads();
    if (threadIdx.x < Rule::kCols) {
        const int e = threadIdx.x;
        partials[(size_t)blockIdx.x * kSumsStride + e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
    }
}

// sum the per-block partial rows in a fixed order -> st->sums[0..27]; sums[28] = count.
// kFinishThreads threads = G row groups x 32 columns: every load instruction reads whole
// 256-byte rows, thread (g, e) adds rows g, g+G, ... of column e with sixteen loads in flight,
// then the G groups are added in order.  Must be called by the whole workgroup.
// (kFinishThreads = 1024 is defined in loop_plan.h: the host plans its launches with it)
constexpr int kFinishGroups = kFinishThreads / 32;

// Counted (icp_gated.h): column 28 of the partial rows holds each block's number of kept rows; their fixed-order sum
// is the count, and n_local is not looked at.  Cols (icp_robust.h): the columns summed -- 30 there, the weight sum in
// column 28 and the kept rows in column 29.
template <bool Counted = false, int Cols = (Counted ? 29 : 28)>
__device__ inline void finish_sums(const double *__restrict__ partials, int nblocks, int n_local,
                                   IcpState *st)
{
    __shared__ double fs[kFinishGroups][32];
    constexpr int G = kFinishGroups;
    const int e = threadIdx.x & 31, g = threadIdx.x >> 5;
    // U partial sums per thread = U loads in flight: the kernel is a chain of memory round trips
    // (1,563 rows at 100k points: 49 per thread, 4 rounds instead of 13 with U = 4)
    constexpr int U = 16;
    double acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0.0;
    // Every round's loads are UNCONDITIONAL (a clamped row, its value dropped by a select: acc + 0.0 is acc, no slot ever
    // holds -0.0) so that they are all in flight together in the last, partial round too.  Written with a guard per load that
    // round was a chain of dependent round trips -- and below 481 rows it is the only round: eight trips for the 250 rows
    // of a filtered scan, four for the 98 group sums of C3.  Only as many slots as the launch's rows fill are loaded (4, 8
    // or 16: a load instruction costs the CU's address unit 16 cycles whether its lanes' rows are clamped or not -- with
    // all sixteen slots always loaded, C3's step kernel lost 0.5 us where the filtered scan's gained 0.5).
    const int last = nblocks - 1;
    auto rounds = [&](auto slots) {
        constexpr int S = decltype(slots)::value;
        for (int b = g; b < nblocks; b += U * G) {
            double v[S];
#pragma unroll
            for (int u = 0; u < S; ++u) {
                const int bb = b + u * G;
                v[u] = partials[(size_t)(bb < nblocks ? bb : last) * kSumsStride + e];
            }
#pragma unroll
            for (int u = 0; u < S; ++u) acc[u] += (b + u * G < nblocks) ? v[u] : 0.0;
        }
    };
    if (nblocks <= 4 * G) rounds(std::integral_constant<int, 4>());
    else if (nblocks <= 8 * G) rounds(std::integral_constant<int, 8>());
    else rounds(std::integral_constant<int, U>());
#pragma unroll
    for (int w = U / 2; w > 0; w >>= 1) // fixed pairwise order
#pragma unroll
        for (int u = 0; u < w; ++u) acc[u] += acc[u + w];
    fs[g][e] = acc[0];
    __syncthreads();
    if (threadIdx.x < Cols) {
        double s = fs[0][e];
        for (int k = 1; k < G; ++k) s += fs[k][e];
        st->sums[e] = s;
    }
    if (!Counted && threadIdx.x == 0) st->sums[28] = (double)n_local;
}

// A second level for the sums of very many partial rows (round 4): a resolve workgroup leaves one row per 64 queries --
// 15,625 at 1M rows -- and every workgroup of the step kernel summed them all (4 MB through each of its CUs).  From
// kSumTreeFrom rows on, this small kernel first adds the rows in groups of kSumGroup, in index order: the step kernels sum
// ceil(nblocks / kSumGroup) rows.  A kernel of its own, not a hand-off inside the resolve kernel: with the last workgroup
// of a group adding the group's rows behind agent-scope fences the resolve took 170 us instead of 27 at C3 (a release
// writes the XCD's L2 back, an acquire drops the CU's L1, once per workgroup and seven workgroups to a CU), and the
// fence-free sc1 form is measured for one workgroup per CU only (MI355X_MICROARCH.md).  A launch boundary costs ~3 us and
// the step kernel's sum of C3's 1,563 rows 6.7: measured at C3, default engine, 30 iterations, same box: 9,614 -> 9,810
// iterations/s with the threshold at 1,024 rows (the sums' order of additions differs on either side of it, inside every
// tolerance of the tests).
// (kSumGroup = 16 and kSumTreeFrom = 1024 are defined in loop_plan.h: the host plans its launches with them)
// Lean passes (list_reuse.h, "lean passes"; `slot` null: none of this): k_sum_groups of pass p sits behind the mover of
// pass p - 1 and in front of the mover of pass p, so ONE MORE workgroup of it can count the rows pass p wanted listed from
// the words that mover left (RowBounds::mask) without racing their writer, and tell the host: (ticket << 32) | count in a
// host-mapped word, one relaxed system-scope store like publish_progress -- the host reads this one word only.  `first`: a
// call's first pass, whose words no mover has written yet, reports every row.  In a lean pass with profiling on
// (`stat_rows` non-null) the same workgroup leaves the pass's statistics, which k_row_list leaves in a full one.
struct WantPublish {
    unsigned long long *slot;       // host-mapped
    unsigned ticket;
    int n, first;
    const unsigned long long *mask; // [(n + 63) / 64]
    const unsigned long long *cert; // the match margin's words (or null)
    unsigned *stat_rows, *stat_cert;
    // solo passes (solo_pass.h; null: none of this): a second host-mapped word, (ticket << 32) | the rows of pass p that are
    // NOT in `cert` -- every row in a call's first pass
    unsigned long long *uncert = nullptr;
};
__device__ __forceinline__ void publish_want(const WantPublish &wp)
{
    __shared__ unsigned part[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (wp.n + 63) / 64;
    const bool certs = (wp.stat_cert || wp.uncert) && wp.cert;
    const unsigned want = wp.first ? 0u : wave_scan_incl((unsigned)row_list_count(wp.mask, tid, nw, 256));
    const unsigned sure = certs && !wp.first ? wave_scan_incl((unsigned)row_list_count(wp.cert, tid, nw, 256)) : 0u;
    if (lane == 63) part[0][wave] = want, part[1][wave] = sure;
    __syncthreads();
    if (tid == 0) {
        const unsigned w = wp.first ? (unsigned)wp.n : (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
        __hip_atomic_store(wp.slot, ((unsigned long long)wp.ticket << 32) | w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (wp.stat_rows) *wp.stat_rows = w;
        const unsigned c = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
        if (certs && wp.stat_cert) *wp.stat_cert = c;
        if (wp.uncert)
            __hip_atomic_store(wp.uncert, ((unsigned long long)wp.ticket << 32) | ((unsigned)wp.n - (certs ? c : 0u)), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
__global__ __launch_bounds__(256) void k_sum_groups(const double *__restrict__ rows, int nblocks, double *__restrict__ rows2,
                                                    const IcpState *__restrict__ st, const WantPublish wp = WantPublish{})
{
    if (st && st->done) return;
    if (wp.slot && blockIdx.x == gridDim.x - 1) { // (the workgroup behind those of the sums)
        publish_want(wp);
        return;
    }
    const int e = threadIdx.x & 31, grp = blockIdx.x * 8 + (threadIdx.x >> 5);
    const int r0 = grp * kSumGroup;
    if (r0 >= nblocks || e >= kNumSums) return;
    const int members = nblocks - r0 < kSumGroup ? nblocks - r0 : kSumGroup;
    double v[kSumGroup];
#pragma unroll
    for (int r = 0; r < kSumGroup; ++r) v[r] = r < members ? rows[(size_t)(r0 + r) * kSumsStride + e] : 0.0; // (all in flight)
    double s = v[0];
#pragma unroll
    for (int r = 1; r < kSumGroup; ++r) s += v[r];
    rows2[(size_t)grp * kSumsStride + e] = s;
}

// error, convergence tests, solve, accumulate (icp.hpp:206-231 / 251-255)
__device__ inline void step_update(IcpState *st, double *history, int final_pass)
{
    if (st->done) {
        if (final_pass && !st->finalized) {
            // the loop broke on convergence: the source has not moved since the last
            // evaluation, so the reference's post-loop pass (icp.hpp:235-252) recomputes
            // exactly last_error
            st->final_error = st->last_error;
            if (history && st->hist_len < st->max_hist) history[st->hist_len] = st->last_error;
            st->hist_len += 1;
            st->finalized = 1;
        }
        return;
    }
    const double error = __dsqrt_rn(st->sums[27] / st->sums[28]);
    if (history && st->hist_len < st->max_hist) history[st->hist_len] = error;
    st->hist_len += 1;
    st->last_error = error;
    if (final_pass) {
        st->final_error = error;
        st->done = 1;
        return;
    }
    st->loops += 1;
    if (error < st->min_error || fabs(st->prev_error - error) < st->tolerance) { // icp.hpp:210-213, 214-217
        st->converged = 1;
        st->done = 1;
        // The post-loop pass of a loop that broke here restates this very error (the source has not moved:
        // icp.hpp:235-252 on unchanged data).  It is entered into the history NOW, so that a host that has seen the
        // loop end need not queue a post-loop pass at all.
        st->final_error = error;
        if (history && st->hist_len < st->max_hist) history[st->hist_len] = error;
        st->hist_len += 1;
        st->finalized = 1;
        return;
    }
    double x[6];
    ldlt6_solve(st->sums, x);       // icp.hpp:120
    twist_to_transform(x, st->delta);    // icp.hpp:123-143
    mul44(st->delta, st->total, st->total); // icp.hpp:229
    st->prev_error = error;              // icp.hpp:231
}

// step_update by the workgroup's first WAVE (all 64 lanes call it, `st` in LDS): the bookkeeping is lane 0's, the solve
// and the 4x4 product are spread over the lanes (ldlt6_solve_wave, mul44_wave), Rodrigues is computed by every lane alike.
// Same operations on every value as step_update -> same bits; ~2.6 instead of 4.7 us between the sums and the moved rows
// of every iteration (scripts/micro/step_clocks.hip).
__device__ inline void step_update_wave(IcpState *st, double *history, int final_pass, int lane)
{
    const bool l0 = lane == 0;
    if (st->done) {
        if (l0 && final_pass && !st->finalized) {
            st->final_error = st->last_error;
            if (history && st->hist_len < st->max_hist) history[st->hist_len] = st->last_error;
            st->hist_len += 1;
            st->finalized = 1;
        }
        return;
    }
    const double error = __dsqrt_rn(st->sums[27] / st->sums[28]);
    const double prev_error = st->prev_error;
    const bool stop = error < st->min_error || fabs(prev_error - error) < st->tolerance; // icp.hpp:210-213, 214-217
    const int hist_len = st->hist_len, max_hist = st->max_hist;
    __builtin_amdgcn_wave_barrier();
    if (l0) {
        if (history && hist_len < max_hist) history[hist_len] = error;
        st->hist_len = hist_len + 1;
        st->last_error = error;
        if (final_pass) {
            st->final_error = error;
            st->done = 1;
        } else {
            st->loops += 1;
            if (stop) { // (the post-loop entry is made now: see step_update)
                st->converged = 1;
                st->done = 1;
                st->final_error = error;
                if (history && hist_len + 1 < max_hist) history[hist_len + 1] = error;
                st->hist_len = hist_len + 2;
                st->finalized = 1;
            } else {
                st->prev_error = error; // icp.hpp:231
            }
        }
    }
    if (final_pass || stop) return;
    double x[6], T[16];
    ldlt6_solve_wave(st->sums, x, lane); // icp.hpp:120
    twist_to_transform(x, T);            // icp.hpp:123-143
    if (l0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) st->delta[e] = T[e];
    }
    __builtin_amdgcn_wave_barrier();
    mul44_wave(st->delta, st->total, st->total, lane); // icp.hpp:229
}

// single GPU: final sum + step in one launch
// `progress` (may be null) is one word of host-mapped memory per iteration slot: the device
// publishes (iteration + 1) * 2 + done there, so the host can stop queueing iterations
// without any copy or event in the stream.
__device__ __forceinline__ void publish_progress(int *progress, int ticket, int done)
{
    // relaxed: the host reads this one word only (results are read after a stream synchronisation);
    // a release here would write the L2 back first, microseconds on every iteration's critical path
    if (progress) __hip_atomic_store(progress, ticket * 2 + (done ? 1 : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The state is staged in LDS for the serial part: step_update touches ~100 of its words one
// after the other, and each would otherwise be a round trip to device memory by a lone thread.
static_assert(sizeof(IcpState) % 8 == 0, "IcpState is copied as 64-bit words");
__device__ __forceinline__ void state_copy(void *dst, const void *src)
{
    const unsigned long long *s = static_cast<const unsigned long long *>(src);
    unsigned long long *d = static_cast<unsigned long long *>(dst);
    for (unsigned w = threadIdx.x; w < sizeof(IcpState) / 8; w += blockDim.x) d[w] = s[w];
}

__device__ inline void step_no_pairs(IcpState *st, double *history, int final_pass); // (icp_gated.h)

// k_finish_step, k_finish_step_gated, k_finish_step_robust: one body.  A counted rule takes the count from the partial rows'
// column 28 (n_local is not looked at) and has the no-pairs rule in front of the step (icp_gated.h).
template <class Rule>
__device__ __forceinline__ void finish_step_rows(const double *__restrict__ partials, int nblocks, int n_local, IcpState *st,
                                                 double *history, int final_pass, int *progress, int ticket)
{
    __shared__ IcpState ls, sums; // `sums`: only its sums[] are used
    // the state and the partial rows are requested together (one round trip instead of two); the
    // sums are taken over only if the loop has not ended
    state_copy(&ls, st);
    finish_sums<Rule::kCounted, Rule::kCols>(partials, nblocks, n_local, &sums);
    __syncthreads();
    constexpr int taken = Rule::kCols > kNumSums ? Rule::kCols : kNumSums;
    if (!ls.done && threadIdx.x < taken) ls.sums[threadIdx.x] = sums.sums[threadIdx.x];
    __syncthreads();
    if (threadIdx.x < 64) {
        if constexpr (Rule::kCounted) {
            const bool none = !ls.done && !(ls.sums[28] > 0.0); // wave-uniform
            __builtin_amdgcn_wave_barrier();
            if (none) {
                if (threadIdx.x == 0) step_no_pairs(&ls, history, final_pass);
            } else {
                step_update_wave(&ls, history, final_pass, threadIdx.x);
            }
        } else {
            step_update_wave(&ls, history, final_pass, threadIdx.x);
        }
        if (threadIdx.x == 0) publish_progress(progress, ticket, ls.done);
    }
    __syncthreads();
    state_copy(st, &ls);
}

__global__ __launch_bounds__(kFinishThreads) void k_finish_step(const double *__restrict__ partials,
                                                     int nblocks, int n_local, IcpState *st,
                                                     double *history, int final_pass, int *progress,
                                                     int ticket)
{
    finish_step_rows<RuleNone>(partials, nblocks, n_local, st, history, final_pass, progress, ticket);
}

// multi GPU: k_finish -> ncclAllReduce(st->sums, kNumExchanged) -> k_step
__global__ __launch_bounds__(kFinishThreads) void k_finish(const double *__restrict__ partials, int nblocks,
                                                int n_local, IcpState *st)
{
    if (st->done) {
        // keep the all-reduce operands finite and identical on every rank
        if (threadIdx.x < kNumSums) st->sums[threadIdx.x] = 0.0;
        if (threadIdx.x == 0) st->sums[kDoneSlot] = 1.0;
        return;
    }
    finish_sums(partials, nblocks, n_local, st);
    if (threadIdx.x == 0) st->sums[kDoneSlot] = 0.0;
}

// The word published to the host carries the AGREED end of the loop: the number of ranks that
// entered this iteration with `done` set (decided one step earlier) came through the exchange
// as an exact integer.  All of them: the loop has ended everywhere, the hosts stop queueing at
// the same iteration and therefore queue the same number of collectives.  Some but not all
// (differing configs, or an all-reduce that did not hand every rank the same bits): every rank
// sees the same count, flags the error and ends its loop at this same iteration.
__global__ __launch_bounds__(64) void k_step(IcpState *st, double *history, int final_pass, int *progress, int ticket,
                                             int n_ranks)
{
    __shared__ IcpState ls;
    state_copy(&ls, st);
    __syncthreads();
    if (threadIdx.x < 64) { // the first wave (step_update_wave)
        const double ndone = ls.sums[kDoneSlot];
        const bool all = ndone == (double)n_ranks, some = ndone > 0.0 && !all;
        if (some && threadIdx.x == 0) {
            ls.error = 1;
            ls.done = 1;
        }
        __builtin_amdgcn_wave_barrier();
        step_update_wave(&ls, history, final_pass, threadIdx.x);
        if (threadIdx.x == 0) publish_progress(progress, ticket, all || some);
    }
    __syncthreads();
    state_copy(st, &ls);
}
// ---- moving the rows (icp.hpp:174-176, 225-226), with the next pass's bounds ---------------------------------------
// What the bounded correspondence search (nn_bounded.h) wants to know about a moved row before it starts: the exact squared
// distance to the target the row was matched with one pass ago, and its fp32 images rounded up.  tgt == nullptr: nothing.
//
// List reuse (xb != nullptr; nn_bounded.h, "Keeping a row's list"): a row's list of slots is built at a position x_b for a
// listing radius R_b -- every slot that may hold a target within R_b of x_b is listed.  At a later pass the row sits at y,
// d = |y - x_b|, and every target that can still be its nearest neighbour is within sqrt(ub) of y, hence within
// sqrt(ub) + d of x_b: while sqrt(ub) + d <= R_b (with a margin for the fp64 roundings of both sides) the kept list is a
// superset of what a new one would list, and the exact resolve returns the same bits from it.  Such a row keeps its
// list (cnt / ent untouched); any other row is listed again for R_b = sqrt(ub) + 2 skin.  The coarse pass runs over the
// rows listed again and over no other: a wave of the kernel that moves the rows holds 64 consecutive rows, and one lane
// stores the wave's ballot of "listed again" as the word of that group of rows (`mask`: every group's word in every pass,
// zeros too, so nothing is ever cleared); k_row_list below packs the set bits' rows, in ascending order, into the list
// k_nn_coarse_bounded takes its rows from (nn_mfma.h, RowsListed).  A row that keeps its list is not in it, and costs the
// coarse pass nothing.
// (kNnEntCap = 8 list words per row, and the records RowList and RowScan: workspace_layout.h)
struct RowBounds {
    const double *tgt; // the target, caller's order
    const int *idx;    // the rows' matches of the pass just finished
    int m;
    double *ub;        // [n] |moved row - tgt[idx]|^2, +Inf without a match
    float *ubf, *sqf;  // [n] the coarse pass's radius^2 in fp32 and its square root, rounded up; NaN / 0 for a row with a
                       // non-finite coordinate, and for one that keeps its list (which the coarse pass never reads: such a
                       // row is not in the packed list)
    int *cnt;          // [n] the row's list length, cleared here for a row listed again by the coming coarse pass
    RowList *xb;       // [n] list reuse (null: every row is listed again, the form before list reuse)
    unsigned long long *mask; // [(n + 63) / 64] list reuse: bit b of word g = row 64 g + b is listed again by the coming pass
    double skin;       // the skin as a fraction of the row's sqrt(ub)
    double loose;      // a list built for more than `loose` x the radius it would be built for now is not kept (0: no limit)
    // The match margin (null: off; on only with list reuse -- list_reuse.h, "the match margin"): the resolve leaves, per row
    // it scans, where it scanned it and how far every target but the winner is from there (g); a row whose kept match is
    // nearer than g less the row's drift since needs no search at all in the coming pass.  Such a row keeps ub, is left
    // with ubf = NaN / sqf = 0, keeps cnt, ent and xb as they are (a list is a standing geometric fact: it may certify
    // again once the margin no longer does), is not in `mask`, and has its bit set in `cert` -- written like `mask`, every
    // group's word in every pass.  Every other row leaves the cover of its list at its new place for the resolve.
    RowScan *scan;            // [n] where the row was last scanned, and its g (NaN: no margin)
    double *cover;            // [n] the coming resolve's: the radius around the row within which its list holds every target
    unsigned long long *cert; // [(n + 63) / 64] bit b of word g = row 64 g + b needs no search in the coming pass
                              // (profiling counts them from these words in k_row_list: once the loop has settled every
                              // wave holds certified rows, and a count per wave here was 1,563 atomics on one word per pass)
};
// B rows of one thread (i0, i0 + stride, ...): every load that does not depend on the pose -- the rows, their previous
// matches' indices, then those targets -- is requested by load(), which the fused kernels call BEFORE their serial step, so
// that the round trips run under it; finish() moves the rows and stores the bounds.
template <int B>
struct RowBatch {
    double x[B], y[B], z[B], tx[B], ty[B], tz[B];
    bool have[B];
    int j[B];
    RowList lb[B]; // list reuse: where the row's list was built, and for which radius
    int c[B];      // ... and its length
    RowScan sc[B]; // the match margin: where the row was last scanned, and its g
    // the rows and their previous matches' indices ...
    __device__ __forceinline__ void load_rows(const double *in, const RowBounds &rb, int i0, int stride, int n,
                                              const unsigned *__restrict__ perm = nullptr)
    {
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int i = i0 + b * stride;
            x[b] = y[b] = z[b] = 0.0;
            j[b] = -1;
            c[b] = 0;
            lb[b] = RowList{0.0, 0.0, 0.0, __builtin_nan("")};
            sc[b] = RowScan{0.0, 0.0, 0.0, __builtin_nan("")};
            if (i < n) {
                const size_t ii = perm ? perm[i] : (unsigned)i;
                x[b] = in[3 * ii], y[b] = in[3 * ii + 1], z[b] = in[3 * ii + 2];
                if (rb.tgt) j[b] = rb.idx[i];
                if (rb.xb) lb[b] = rb.xb[i], c[b] = rb.cnt[i];
                if (rb.scan) sc[b] = rb.scan[i];
            }
        }
    }
    // ... and the matched targets, a round trip that DEPENDS on the indices: a kernel with other loads to issue (the state,
    // the partial rows) calls this after them -- waves issue in order, so behind this gather's wait for the indices those
    // loads would start one round trip late
    __device__ __forceinline__ void load_matches(const RowBounds &rb)
    {
#pragma unroll
        for (int b = 0; b < B; ++b) {
            have[b] = rb.tgt && (unsigned)j[b] < (unsigned)rb.m;
            tx[b] = ty[b] = tz[b] = 0.0;
            if (have[b]) tx[b] = rb.tgt[3 * (size_t)j[b]], ty[b] = rb.tgt[3 * (size_t)j[b] + 1], tz[b] = rb.tgt[3 * (size_t)j[b] + 2];
        }
    }
    __device__ __forceinline__ void load(const double *in, const RowBounds &rb, int i0, int stride, int n,
                                         const unsigned *__restrict__ perm = nullptr)
    {
        load_rows(in, rb, i0, stride, n, perm);
        load_matches(rb);
    }
    // one row of the batch: moved, stored, its bounds and words left for the coming pass; what the caller may go on with
    struct Moved {
        double px, py, pz, ub;             // the moved row and its exact squared distance to its kept match (+Inf: none)
        bool cert;                         // the match margin certified it
        unsigned long long again, sure;    // the wave's words (RowBounds::mask, RowBounds::cert), as stored
    };
    __device__ __forceinline__ Moved finish_row(const int b, const int i, double *out, const RowBounds &rb, const Rigid34 &P) const
    {
        Moved mv{0.0, 0.0, 0.0, __builtin_inf(), false, 0ull, 0ull};
        double px, py, pz;
        P.apply(x[b], y[b], z[b], px, py, pz);
        mv.px = px, mv.py = py, mv.pz = pz;
        out[3 * i] = px;
        out[3 * i + 1] = py;
        out[3 * i + 2] = pz;
        if (rb.tgt) {
            // A row with a NaN or infinite coordinate has no neighbour (kdtree.hpp:125): NaN, under which the coarse pass
            // lists nothing.  No previous match (every target non-finite ...): +Inf, everything is listed.
            double ub = __builtin_inf();
            float ubf = __builtin_nanf(""), sqf = 0.f;
            bool keep = false, cert = false;
            if (__builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(pz)) {
                if (have[b]) ub = sqdist(tx[b], ty[b], tz[b], px, py, pz);
                double r2 = ub; // the radius^2 the coarse pass lists for
                if (rb.xb) {
                    // the certificate (see RowBounds; list_reuse.h).  A list is not kept if it overflowed (cnt > kNnEntCap: the resolve's exhaustive path) or is empty (cnt == 0: a row beyond fp32's
                    // range), nor if R_b is more than `loose` times the radius it would be built for now (a loose list:
                    // slots the resolve would scan for nothing).  R_b NaN (first pass) fails every comparison.
                    const double sq = __builtin_sqrt(ub);
                    if (rb.scan) { // the match margin first: a certified row has nothing to do with its list
                        const double sx = px - sc[b].x, sy = py - sc[b].y, sz = pz - sc[b].z;
                        cert = match_certified(sq, __builtin_sqrt((sx * sx + sy * sy) + sz * sz), sc[b].g);
                    }
                    if (!cert) {
                        const double ex = px - lb[b].x, ey = py - lb[b].y, ez = pz - lb[b].z;
                        const double d = __builtin_sqrt((ex * ex + ey * ey) + ez * ez);
                        const double mx = px - x[b], my = py - y[b], mz = pz - z[b];
                        const double rn = list_radius(sq, __builtin_sqrt((mx * mx + my * my) + mz * mz), rb.skin);
                        keep = c[b] > 0 && c[b] <= kNnEntCap && list_certified(sq, d, lb[b].r) &&
                               (rb.loose <= 0.0 || lb[b].r <= rb.loose * rn);
                        if (!keep) {
                            r2 = rn * rn;
                            rb.xb[i] = RowList{px, py, pz, rn};
                        }
                        if (rb.cover) rb.cover[i] = keep ? list_cover(lb[b].r, d) : list_cover(rn, 0.0);
                    }
                }
                if (!keep && !cert) {
                    ubf = (float)r2;
                    ubf = (double)ubf < r2 ? __uint_as_float(__float_as_uint(ubf) + 1u) : ubf; // (r2 >= 0; Inf stays Inf)
                    sqf = __builtin_amdgcn_sqrtf(ubf);
                    sqf = sqf < 3.0e38f ? __uint_as_float(__float_as_uint(sqf) + 2u) : sqf;   // (1 ulp of v_sqrt_f32 and one more)
                }
            }
            mv.ub = ub, mv.cert = cert;
            rb.ub[i] = ub;
            rb.ubf[i] = ubf;
            rb.sqf[i] = sqf;
            if (!keep && !cert) rb.cnt[i] = 0;
            if (rb.mask) {
                // the wave's rows are 64 consecutive ones from a multiple of 64 (rows past n are not here and leave their
                // bits clear): lane 0 holds the first of them and stores the group's word
                const unsigned long long again = __ballot(!keep && !cert && ubf == ubf);
                if ((i & 63) == 0) rb.mask[i >> 6] = again;
                mv.again = again;
                if (rb.cert) {
                    const unsigned long long sure = __ballot(cert);
                    if ((i & 63) == 0) rb.cert[i >> 6] = sure;
                    mv.sure = sure;
                }
            }
        }
        return mv;
    }
    __device__ __forceinline__ void finish(double *out, const RowBounds &rb, int i0, int stride, int n, const double *T) const
    {
        const Rigid34 P = Rigid34::load(T);
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int i = i0 + b * stride;
            if (i >= n) continue;
            (void)finish_row(b, i, out, rb, P);
        }
    }
};
// Rows per thread and batch.  The fused kernels' grids give a thread ONE row up to 131,072 rows (k_transform: 524,288), so a
// batch only costs registers there, and with the match margin's record a batch of 4 rows no longer fit
// k_finish_step_transform's 128 registers (1,024 threads): 216 dwords spilled, 41 before the record.  At 2: 125 registers,
// nothing spilled (k_step_transform 114, k_transform 81; -Rpass-analysis=kernel-resource-usage).
constexpr int kRowBatch = 2;

// The packed list of the rows listed again, from the words the kernel that moved the rows left (RowBounds::mask):
// list[0] = their number, list[1] = 1 where that is every row (the coarse pass then indexes its rows directly and reads no
// list: none is written), list[kRowListHead ...] = the rows in ascending order -- neighbours in the list are neighbours in
// the rows' Morton order, which the coarse epilogue's short path lives on.  One word per thread.  A workgroup waits for no
// other one: each counts the words below its own itself (12 KB of words per 100k rows, out of the L2), and the rest for the
// total, then scans its own 256 counts and expands its words (list_reuse.h).  No atomics.  Every workgroup thus reads all
// ceil(n / 64) words, quadratic in n / 16,384: 7 workgroups x 12 KB at 100k rows, 62 x 125 KB at 1M rows (not measured there;
// a pass is 29 ms at that size).
// Measured and dropped: the same work at the end of the kernel that moves the rows, by its last workgroup behind a fence and
// a ticket per workgroup -- one launch fewer per iteration, but the fences cost the moving kernel more than the launch:
// C3 at 30 steps 1.11x the parent's rate against 1.43x in this form, and 0.82x against 1.22x at 100 steps (same box,
// alternating; profiles/row_list/).
constexpr int kRowListThreads = 256;
// (kRowListHead = 16 words in front of the list, so that the rows start on a 64-byte line: workspace_layout.h)
// Profiling (`rows_count` non-null): the first workgroup stores the number of rows listed, and with the match margin
// (`cert_count` non-null) it also counts the set bits of the rows' "certified" words (RowBounds::cert) and stores their
// number -- plain stores, no atomics (a count per wave in the kernel that moves the rows was 1,563 atomics on one word).
__global__ __launch_bounds__(kRowListThreads) void k_row_list(const unsigned long long *__restrict__ mask, int n, int *__restrict__ list,
                                                              const IcpState *__restrict__ st,
                                                              const unsigned long long *__restrict__ cert = nullptr,
                                                              unsigned *__restrict__ cert_count = nullptr,
                                                              unsigned *__restrict__ rows_count = nullptr)
{
    if (st->done) return; // (the rows were not moved and the coarse pass will not run)
    __shared__ int part[4][kRowListThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nw = (n + 63) / 64, g0 = blockIdx.x * kRowListThreads, g = g0 + tid;
    const unsigned long long w = g < nw ? mask[g] : 0ull;
    const int mine = row_list_popcount(w);
    const unsigned below = wave_scan_incl((unsigned)row_list_count(mask, tid, g0, kRowListThreads));
    const unsigned above = wave_scan_incl((unsigned)row_list_count(mask, g0 + kRowListThreads + tid, nw, kRowListThreads));
    const unsigned incl = wave_scan_incl((unsigned)mine);
    if (lane == 63) part[0][wave] = (int)below, part[1][wave] = (int)above, part[2][wave] = (int)incl;
    if (cert_count && blockIdx.x == 0) {
        const unsigned sure = wave_scan_incl((unsigned)row_list_count(cert, tid, nw, kRowListThreads));
        if (lane == 63) part[3][wave] = (int)sure;
    }
    __syncthreads();
    if (cert_count && blockIdx.x == 0 && tid == 0) {
        int c = 0;
        for (int v = 0; v < kRowListThreads / 64; ++v) c += part[3][v];
        *cert_count = (unsigned)c;
    }
    int at = 0, total = 0;
#pragma unroll
    for (int v = 0; v < kRowListThreads / 64; ++v) {
        at += part[0][v] + (v < wave ? part[2][v] : 0);
        total += part[0][v] + part[1][v] + part[2][v];
    }
    if (blockIdx.x == 0 && tid == 0) {
        list[0] = total, list[1] = total == n;
        if (rows_count) *rows_count = (unsigned)total;
    }
    if (total == n) return;
    row_list_expand(w, g, list + kRowListHead, at + (int)incl - mine);
}


// multi GPU, one launch fewer per iteration: k_step and k_transform in one kernel.  Every workgroup
// repeats the (deterministic) step from the all-reduced sums on its own LDS copy of the state --
// the same bits in, the same bits out -- and moves its points with the update it has just formed
// (icp.hpp:220-226); workgroup 0 alone records the history entry, publishes the progress word and
// stores the new state.  It stores it into the OTHER of two state buffers: a workgroup that starts
// late must still read the state of before the step, so the loop's kernels alternate between the
// two (`sin` of one iteration is `sout` of the previous one).
__global__ __launch_bounds__(256) void k_step_transform(const double *in, double *out, int n, const IcpState *sin,
                                                        IcpState *sout, double *history, int *progress, int ticket,
                                                        int n_ranks, const RowBounds rb)
{
    __shared__ IcpState ls;
    const int i0 = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256; // (a wave: 64 rows from a multiple of 64, RowBounds::mask)
    RowBatch<kRowBatch> rows;
    rows.load(in, rb, i0, stride, n);
    state_copy(&ls, sin);
    __syncthreads();
    if (threadIdx.x < 64) { // the first wave (step_update_wave)
        const double ndone = ls.sums[kDoneSlot];
        const bool all = ndone == (double)n_ranks, some = ndone > 0.0 && !all;
        if (some && threadIdx.x == 0) {
            ls.error = 1;
            ls.done = 1;
        }
        __builtin_amdgcn_wave_barrier();
        step_update_wave(&ls, blockIdx.x == 0 ? history : nullptr, 0, threadIdx.x);
        if (threadIdx.x == 0 && blockIdx.x == 0) publish_progress(progress, ticket, all || some);
    }
    __syncthreads();
    if (blockIdx.x == 0) state_copy(sout, &ls);
    if (ls.done) return; // the loop ended before or in this step: the source stays where it is (icp.hpp:210-217)
    for (int base = i0; base < n; base += kRowBatch * stride) {
        if (base != i0) rows.load(in, rb, base, stride, n);
        rows.finish(out, rb, base, stride, n, ls.delta);
    }
}

// single GPU, two launches fewer per iteration: k_finish_step and k_transform in one kernel, on the
// same footing as k_step_transform.  EVERY workgroup sums all partial rows itself (same rows, same
// order, same bits: a 400 KB read out of the L2 at 100k points, 50 KB at the 7k points of a filtered
// scan), repeats the step on its own LDS copy of the state and moves its share of the points;
// workgroup 0 alone records the history entry, publishes the progress word and stores the new state
// into the other state buffer.  No workgroup waits for another one.
__global__ __launch_bounds__(kFinishThreads) void k_finish_step_transform(
    const double *__restrict__ partials, int nblocks, int n_local, const double *in, double *out, int n,
    const IcpState *sin, IcpState *sout, double *history, int *progress, int ticket, const RowBounds rb)
{
    __shared__ IcpState ls, sums; // `sums`: only its sums[] are used
    // The kernel is a chain of memory round trips, so everything that does not depend on the state
    // is requested first: this thread's first rows (with their previous matches), and the partial rows (summed whether
    // or not the loop has ended; the sums are taken over only if it has not, like k_finish_step).
    static_assert(kFinishThreads % 64 == 0, "a wave's rows start at a multiple of 64 (RowBounds::mask)");
    const int i0 = blockIdx.x * kFinishThreads + threadIdx.x, stride = gridDim.x * kFinishThreads;
    RowBatch<kRowBatch> rows;
    rows.load_rows(in, rb, i0, stride, n);
    state_copy(&ls, sin);
    finish_sums(partials, nblocks, n_local, &sums);
    __syncthreads();
    rows.load_matches(rb); // (in flight under the step)
    if (!ls.done && threadIdx.x < kNumSums) ls.sums[threadIdx.x] = sums.sums[threadIdx.x];
    __syncthreads();
    if (threadIdx.x < 64) { // the first wave (step_update_wave)
        step_update_wave(&ls, blockIdx.x == 0 ? history : nullptr, 0, threadIdx.x);
        if (threadIdx.x == 0 && blockIdx.x == 0) publish_progress(progress, ticket, ls.done);
    }
    __syncthreads();
    if (blockIdx.x == 0) state_copy(sout, &ls);
    if (ls.done) return; // the loop ended before or in this step: the source stays where it is (icp.hpp:210-217)
    for (int base = i0; base < n; base += kRowBatch * stride) {
        if (base != i0) rows.load(in, rb, base, stride, n);
        rows.finish(out, rb, base, stride, n, ls.delta);
    }
}

// one-shot solve for icpmi_solve_point_to_plane (icp.hpp:89-144)
__global__ __launch_bounds__(kFinishThreads) void k_finish_solve(const double *__restrict__ partials,
                                                      int nblocks, int n_local, IcpState *st)
{
    finish_sums(partials, nblocks, n_local, st);
    __syncthreads();
    if (threadIdx.x == 0) {
        double x[6];
            ldlt6_solve(st->sums, x);
        twist_to_transform(x, st->delta);
    }
}

// out = in * R^T + t^T with T read from device memory (st->delta or a staged matrix).
// which: 0 = st->delta, 1 = st->total
// perm (may be null): out row i is made from in row perm[i] (the ICP loop takes its source rows in Morton order)
__global__ __launch_bounds__(256) void k_transform(const double *in, double *out, int n,
                                                   const IcpState *__restrict__ st, int which,
                                                   int honour_done, const unsigned *__restrict__ perm = nullptr,
                                                   const RowBounds rb = RowBounds{})
{
    if (honour_done && st->done) return;
    const double *T = which ? st->total : st->delta;
    const int i0 = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    RowBatch<kRowBatch> rows;
    for (int base = i0; base < n; base += kRowBatch * stride) {
        rows.load(in, rb, base, stride, n, perm);
        rows.finish(out, rb, base, stride, n, T);
    }
}

} // namespace icpmi
