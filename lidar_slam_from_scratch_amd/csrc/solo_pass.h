// solo_pass.h -- a settled pass of the all-pairs ICP loop as ONE launch (LoopPlan::solo_on, loop_plan.h).
//
// Once the match margin certifies every row (list_reuse.h), a pass of the loop searches nothing: k_nn_resolve_bounded<true>
// reads each row and its kept match back, gathers one normal, forms the 28 normal-equation terms and leaves a partial row per
// 64 rows; k_sum_groups adds those in groups of 16; k_finish_step_transform sums the group rows, steps and moves the rows.
// Three launches over data the mover held in registers a launch earlier.  k_finish_step_transform_solo is that mover, S(p),
// doing for its own rows what the resolve and k_sum_groups of pass p + 1 would have done, so that pass p + 1 launches only
// its own tail:
//   - wave w of workgroup b of the mover holds rows 1024 b + 64 w ... + 63: the rows of resolve workgroup 16 b + w, hence of
//     partial row 16 b + w, and k_sum_groups adds partial rows 16 b ... 16 b + 15 into group row b.  One mover workgroup
//     owns exactly the rows of one group sum and writes it itself, with LDS and a workgroup barrier: no workgroup waits for
//     another, there are no fences.  The additions are those of resolve_finish (nn_mfma.h) and k_sum_groups (kernels.h) in
//     their order -- per 16 rows the columns over rows 0-7 and 8-15, each from 0.0, first half + second half; per 64 rows
//     ((W0 + W1) + W2) + W3; per 1,024 rows P0, += P1 ... P15 -- so group row b has the bits the three launches leave.
//   - a row the mover did NOT certify is searched here, by the resolve's exhaustive path from its incumbent (nn_bounded.h,
//     `over`: split boxes, then scan_split, the whole wave on one row at a time; exact, ties to the lowest original index).
//     A host that queues this kernel for a pass that is not settled after all loses time, never a bit.  Such a row stores
//     RowScan{p, NaN} like an `over` row; a row with a non-finite coordinate gets idx = -1 and its terms from target 0.
//   - every workgroup reads ALL group rows of pass p and writes ONE of pass p + 1, so the two alternate between two areas
//     (a late workgroup still reads the old sums), and a workgroup leaves the coming pass's counts -- rows listed again, rows
//     not certified, rows searched here -- in a slot of its own; the next tail's first workgroup (or k_publish_counts) adds
//     the slots in index order and tells the host (WantPublish, kernels.h): S(p + 1) overwrites the rows' words while it runs.
#pragma once
#include "kernels.h"
#include "nn_bounded.h"

namespace icpmi {

constexpr int kSoloWaves = kFinishThreads / 64;
constexpr int kSoloCols = 4;                    // columns of the 28 staged per phase: 64 rows x 4 doubles per wave
constexpr int kSoloPhases = 28 / kSoloCols;
constexpr int kSoloStride = kSoloCols + 1;      // doubles per staged row (5: the eight summing lanes of a column hit four banks pairs, not one)
static_assert(kSoloPhases * kSoloCols == 28, "whole phases");
static_assert(kResolveWW * kResolveQ == 64 && kSumGroup == kSoloWaves, "a wave's rows are a partial row's, a workgroup's a group row's");

// (SoloCounts, one workgroup's counts: workspace_layout.h)

struct SoloPass {
    // the target's search structure, for rows this kernel has to search itself (k_nn_resolve_bounded's arguments)
    const double *sorted;
    const unsigned *perm;
    int ms, splits;
    const SplitFrame *frames;
    const double *nrm;       // the target's normals, caller's order
    int *idx;                // the rows' matches (RowBounds::idx, to be written for a searched row)
    double *groups_out;      // [gridDim.x] the coming pass's group rows
    SoloCounts *counts_out;  // [gridDim.x] the coming pass's counts, a slot per workgroup
    // this pass's counts, left by the solo kernel that ended the pass before (null `want`: k_sum_groups has published them)
    const SoloCounts *counts_in;
    int blocks_in;
    unsigned long long *want, *uncert; // host-mapped: (ticket << 32) | count
    unsigned ticket;
    int n;
    unsigned *stat_rows, *stat_cert, *stat_searched; // profiling (or null)
};

// workgroup slots -> the pass's counts, by one wave; lane 0 tells the host and leaves the statistics
__device__ __forceinline__ void solo_publish(const SoloPass &sp, const int lane)
{
    unsigned w = 0, u = 0, f = 0;
    for (int b = lane; b < sp.blocks_in; b += 64) w += sp.counts_in[b].want, u += sp.counts_in[b].uncert, f += sp.counts_in[b].searched;
    w = wave_scan_incl(w), u = wave_scan_incl(u), f = wave_scan_incl(f); // (integers: any order)
    if (lane == 63) {
        __hip_atomic_store(sp.want, ((unsigned long long)sp.ticket << 32) | w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(sp.uncert, ((unsigned long long)sp.ticket << 32) | u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (sp.stat_rows) *sp.stat_rows = w;
        if (sp.stat_cert) *sp.stat_cert = (unsigned)sp.n - u;
        if (sp.stat_searched) *sp.stat_searched = f;
    }
}

// The counts of a pass behind a solo kernel whose own tail is not one (k_finish_step_transform, or the post-loop
// k_finish_step): one wave in front of that tail.
__global__ __launch_bounds__(64) void k_publish_counts(const IcpState *__restrict__ st, const SoloPass sp)
{
    if (st->done) return;
    solo_publish(sp, threadIdx.x);
}

// term o of a partial row (kernels.h, kNumSums) as a product of two of (J0 ... J5, b): 21 of J^T J, upper, row by row; 6 of
// J^T b; b b
__host__ __device__ constexpr int solo_term_r(int o)
{
    if (o >= 27) return 6;
    if (o >= 21) return o - 21;
    int r = 0;
    for (int base = 0; o >= base + (6 - r); base += 6 - r, ++r) {}
    return r;
}
__host__ __device__ constexpr int solo_term_c(int o)
{
    if (o >= 21) return 6;
    int r = 0, base = 0;
    for (; o >= base + (6 - r); base += 6 - r, ++r) {}
    return r + (o - base);
}
static_assert(solo_term_r(0) == 0 && solo_term_c(5) == 5 && solo_term_r(6) == 1 && solo_term_c(6) == 1 && solo_term_r(20) == 5 &&
                  solo_term_c(20) == 5 && solo_term_r(26) == 5 && solo_term_c(26) == 6 && solo_term_r(27) == 6,
              "resolve_finish's order of terms");

// The terms' arithmetic, operand by operand as k_nn_resolve_bounded's resolve_finish compiles (nn_mfma.h): every value is
// IEEE's whatever the order of a product's or a sum's operands, but where BOTH are NaN -- a row with a non-finite
// coordinate, every row under a NaN pose -- the hardware returns the first operand's NaN, sign and payload, and the normal
// matrix of such a call is compared byte for byte too (tests/test_gpu_solo_passes.py, the NaN / Inf source).  The compiler
// commutes operands as it likes, differently in the two kernels, so they are pinned here: J = p x n as (p_a n_b) - (p_b n_a),
// e = q - p, b = e2 n2 + (e0 n0 + e1 n1), J_r J_c with r <= c, b J_r, b b.
__device__ __forceinline__ double solo_mul(double a, double b)
{
    double r;
    asm("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double solo_add(double a, double b)
{
    double r;
    asm("v_add_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double solo_sub(double a, double b)
{
    double r;
    asm("v_add_f64 %0, %1, -%2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// term o from (J0 ... J5, b): the row's b goes first where it is a factor
template <int O> __device__ __forceinline__ double solo_term(const double (&J7)[7])
{
    constexpr int r = solo_term_r(O), c = solo_term_c(O);
    return (c == 6 && r < 6) ? solo_mul(J7[6], J7[r]) : solo_mul(J7[r], J7[c]);
}

// Columns 4 PH ... 4 PH + 3 of the wave's 64 rows: staged, summed per block of 16 rows and per 64 in resolve_finish's order,
// into the wave's partial row `red`.  Lane 4 k + c sums column c over rows 8 k ... 8 k + 7 from 0.0; lanes 8 v + c then hold
// resolve wave v's first half + second half, and lanes c < 4 add the four in order.  No LDS crossbar trip (lane_xor).
template <int PH>
__device__ __forceinline__ void solo_phases(double (*__restrict__ stg)[kSoloStride], double *__restrict__ red, const double (&J7)[7], const int lane)
{
    stg[lane][0] = solo_term<4 * PH>(J7);
    stg[lane][1] = solo_term<4 * PH + 1>(J7);
    stg[lane][2] = solo_term<4 * PH + 2>(J7);
    stg[lane][3] = solo_term<4 * PH + 3>(J7);
    __builtin_amdgcn_wave_barrier();
    const int k = (lane >> 2) & 7, c = lane & 3; // (lanes 32-63 repeat lanes 0-31: nothing of theirs is stored)
    double v = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) v += stg[8 * k + r][c];
    v += lane_xor<4>(v);                  // lanes 8 v + c: rows 0-7 + rows 8-15 of resolve wave v
    const double a = lane_xor<8>(v);      // lanes c: W1, lanes 16 + c: W3
    const double w2 = lane_xor<16>(v), w3 = lane_xor<16>(a);
    if (lane < kSoloCols) red[4 * PH + lane] = ((v + a) + w2) + w3;
    __builtin_amdgcn_wave_barrier();
    if constexpr (PH + 1 < kSoloPhases) solo_phases<PH + 1>(stg, red, J7, lane);
}

// S(p): k_finish_step_transform for a source of one row per thread (n <= gridDim.x * kFinishThreads), every value it
// stores unchanged, then the terms and the group sum of pass p + 1 for the workgroup's rows.
__global__ __launch_bounds__(kFinishThreads) void k_finish_step_transform_solo(
    const double *__restrict__ partials, int nblocks, int n_local, const double *in, double *out, int n, const IcpState *sin,
    IcpState *sout, double *history, int *progress, int ticket, const RowBounds rb, const SoloPass sp)
{
    __shared__ IcpState ls, sums; // `sums`: only its sums[] are used
    __shared__ double stage[kSoloWaves][64][kSoloStride];
    __shared__ double red[kSoloWaves][28];
    __shared__ unsigned cnts[kSoloWaves][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * kFinishThreads + threadIdx.x;
    const bool valid = i < n;
    RowBatch<1> rows;
    rows.load_rows(in, rb, i, 0, n);
    state_copy(&ls, sin);
    finish_sums(partials, nblocks, n_local, &sums);
    __syncthreads();
    rows.load_matches(rb); // (in flight under the step, and the kept match's normal with it)
    int jq = rows.have[0] ? rows.j[0] : -1; // the target q and n are of
    double q0 = rows.tx[0], q1 = rows.ty[0], q2 = rows.tz[0], n0 = 0.0, n1 = 0.0, n2 = 0.0;
    if (jq >= 0) n0 = sp.nrm[3 * (size_t)jq], n1 = sp.nrm[3 * (size_t)jq + 1], n2 = sp.nrm[3 * (size_t)jq + 2];
    const int was_done = ls.done;
    if (!was_done && threadIdx.x < kNumSums) ls.sums[threadIdx.x] = sums.sums[threadIdx.x];
    __syncthreads();
    if (threadIdx.x < 64) { // the first wave (step_update_wave)
        step_update_wave(&ls, blockIdx.x == 0 ? history : nullptr, 0, threadIdx.x);
        if (threadIdx.x == 0 && blockIdx.x == 0) publish_progress(progress, ticket, ls.done);
    } else if (wave == 1 && blockIdx.x == 0 && sp.want && !was_done) {
        solo_publish(sp, lane); // (like k_sum_groups: not once the loop has ended)
    }
    __syncthreads();
    if (blockIdx.x == 0) state_copy(sout, &ls);
    if (ls.done) return; // the loop ended before or in this step: the source stays where it is (icp.hpp:210-217)

    const Rigid34 P = Rigid34::load(ls.delta);
    RowBatch<1>::Moved mv{0.0, 0.0, 0.0, __builtin_inf(), false, 0ull, 0ull};
    if (valid) mv = rows.finish_row(0, i, out, rb, P);

    // the rows not certified: the resolve's incumbent, then its exhaustive search (nn_bounded.h, `over`)
    const double kMax = 1.7976931348623157e308;
    const bool look = valid && finite3(mv.px, mv.py, mv.pz);
    int bj = (look && rows.have[0]) ? rows.j[0] : 0x7fffffff;
    double bd = bj == 0x7fffffff ? kMax : mv.ub;
    const unsigned long long searched = __ballot(look && !mv.cert);
    unsigned long long pend = searched;
    while (pend) { // rare; wave-uniform loop
        const int L = __ffsll((long long)pend) - 1;
        pend &= pend - 1;
        const double qx = __shfl(mv.px, L, 64), qy = __shfl(mv.py, L, 64), qz = __shfl(mv.pz, L, 64);
        double qd = __shfl(bd, L, 64);
        int qj = __shfl(bj, L, 64);
        for (int s0 = 0; s0 < sp.splits; s0 += 64) {
            bool keep = false;
            if (s0 + lane < sp.splits) {
                const SplitFrame &f = sp.frames[s0 + lane];
                double lb = 0.0;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double q = px_sel(a, qx, qy, qz);
                    const double g1 = f.lo[a] - q, g2 = q - f.hi[a];
                    const double g = g1 > g2 ? (g1 > 0.0 ? g1 : 0.0) : (g2 > 0.0 ? g2 : 0.0);
                    lb += g * g;
                }
                keep = !(lb * (1.0 - 1e-9) > qd); // (an empty split's box is inverted: infinitely far)
            }
            unsigned long long smask = __ballot(keep);
            while (smask) {
                const int sL = s0 + __ffsll((long long)smask) - 1;
                smask &= smask - 1;
                scan_split<kResolveScanBatch>(sp.sorted, sp.perm, rb.m, sp.ms, reinterpret_cast<const double *>(sp.frames + sp.splits), sL,
                                              qx, qy, qz, qd, lane, qd, qj);
            }
        }
        if (lane == L) {
            bd = qd;
            bj = qj;
        }
    }
    if (valid && !mv.cert) { // what the resolve leaves of a row it did not find certified
        sp.idx[i] = bj == 0x7fffffff ? -1 : bj;
        rb.scan[i] = RowScan{mv.px, mv.py, mv.pz, __builtin_nan("")};
    }
    if (lane == 0) {
        const int in_wave = n - (i < n ? i : n) < 64 ? n - (i < n ? i : n) : 64;
        cnts[wave][0] = (unsigned)__popcll(mv.again);
        cnts[wave][1] = (unsigned)in_wave - (unsigned)__popcll(mv.sure);
        cnts[wave][2] = (unsigned)__popcll(searched);
    }

    // the row's terms (resolve_finish: J = p x n, b = (e0 n0 + e1 n1) + e2 n2; a row past the end adds +0.0 products)
    double J7[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (valid) {
        const int j = (unsigned)bj < (unsigned)rb.m ? bj : 0;
        if (j != jq) { // searched, or without a match: target 0 or the new one
            q0 = rb.tgt[3 * (size_t)j], q1 = rb.tgt[3 * (size_t)j + 1], q2 = rb.tgt[3 * (size_t)j + 2];
            n0 = sp.nrm[3 * (size_t)j], n1 = sp.nrm[3 * (size_t)j + 1], n2 = sp.nrm[3 * (size_t)j + 2];
        }
        J7[0] = solo_sub(solo_mul(mv.py, n2), solo_mul(mv.pz, n1)); // p x n, icp.hpp:105
        J7[1] = solo_sub(solo_mul(mv.pz, n0), solo_mul(mv.px, n2));
        J7[2] = solo_sub(solo_mul(mv.px, n1), solo_mul(mv.py, n0));
        J7[3] = n0;
        J7[4] = n1;
        J7[5] = n2;
        const double e0 = solo_sub(q0, mv.px), e1 = solo_sub(q1, mv.py), e2 = solo_sub(q2, mv.pz);
        J7[6] = solo_add(solo_mul(e2, n2), solo_add(solo_mul(e0, n0), solo_mul(e1, n1))); // (e0 n0 + e1 n1) + e2 n2, icp.hpp:116
    }
    solo_phases<0>(stage[wave], red[wave], J7, lane);
    __syncthreads();
    if (threadIdx.x < 28) { // k_sum_groups' order over the workgroup's sixteen partial rows
        const int e = threadIdx.x;
        double s = red[0][e];
#pragma unroll
        for (int w = 1; w < kSoloWaves; ++w) s += red[w][e];
        sp.groups_out[(size_t)blockIdx.x * kSumsStride + e] = s;
    } else if (threadIdx.x == 32) {
        SoloCounts c{0u, 0u, 0u, 0u};
        for (int w = 0; w < kSoloWaves; ++w) c.want += cnts[w][0], c.uncert += cnts[w][1], c.searched += cnts[w][2];
        sp.counts_out[blockIdx.x] = c;
    }
}

} // namespace icpmi
