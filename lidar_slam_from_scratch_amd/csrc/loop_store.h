// loop_store.h -- the loop-closure detector's database on the device, as an index over the frames of a global map
// store (icpmi_loop, capi.hip; reference core/loop_closure.hpp:41-148).  An entry is a store frame with the label the
// caller gave it (the node's frame_idx).  Per entry the device holds its 1,200-double Scan Context descriptor and its
// label; the rows stay in the store (global_map.h).
//
//   k_loop_describe    one workgroup per entry added since the last detect: sc_describe (scan_context.h, the body
//                      of k_scan_context) over the entry's rows in the store
//   k_loop_candidates  one workgroup per older entry: the label gap test (loop_closure.hpp:80-82), sc_distance
//                      (the body of k_sc_distances) to the newest entry and the threshold (:86-89).  Passing entries
//                      append (distance, entry) to a host-mapped list; the last workgroup to finish writes the
//                      list's length there too and rearms the counters, so the host waits once and reads only the
//                      candidates.
//   k_loop_candidates_shift  the same pass with sc_distance_shift: each record also carries the smallest column shift
//                      that attains its distance, from which the candidate's verification starts (yaw guess, capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_context.h"

namespace icpmi {

struct LoopJob {
    int64_t row0;  // the entry's first row in the store
    int32_t rows;
    int32_t label; // frame_idx
};
static_assert(sizeof(LoopJob) == 16, "the job table is uploaded as it is");

struct LoopCandidate {
    double dist;
    int64_t entry;
};
static_assert(sizeof(LoopCandidate) == 16, "the host reads the list as it is");

// k_loop_candidates_shift's record: as wide as LoopCandidate (one host list serves both), the shift beside the entry
struct LoopCandidateShift {
    double dist;
    int32_t entry;
    int32_t shift; // 0..59
};
static_assert(sizeof(LoopCandidateShift) == sizeof(LoopCandidate), "the host list holds either record");

// grid = pending entries, entry0 + blockIdx.x being the entry each describes
__global__ __launch_bounds__(1024) void k_loop_describe(const double *__restrict__ store, const LoopJob *__restrict__ jobs,
                                                        int32_t entry0, double *__restrict__ table, int32_t *__restrict__ labels)
{
    const LoopJob j = jobs[blockIdx.x];
    const int64_t e = (int64_t)entry0 + blockIdx.x;
    sc_describe(store + 3 * (size_t)j.row0, j.rows, table + (size_t)e * kScCells);
    if (threadIdx.x == 0) labels[e] = j.label;
}

// grid = q (the entries older than the query q), 64 threads.  counters[0] is the list's length, counters[1] the
// workgroups done; both are 0 on entry and again on exit.  out_n and out point to host-mapped memory (cap >= q).
__global__ __launch_bounds__(64) void k_loop_candidates(const double *__restrict__ table, const int32_t *__restrict__ labels,
                                                        int32_t q, int32_t frame_gap, double threshold,
                                                        unsigned *__restrict__ counters, LoopCandidate *out,
                                                        int64_t *out_n)
{
    const int32_t d = blockIdx.x;
    // label[q] - label[i] < frame_gap: skipped (the labels' difference in 64 bits: no overflow)
    if ((int64_t)labels[q] - (int64_t)labels[d] >= (int64_t)frame_gap) {
        const double dist = sc_distance(table + (size_t)q * kScCells, table + (size_t)d * kScCells);
        if (threadIdx.x == 0 && dist < threshold) { // strict; NaN never passes
            const unsigned slot = atomicAdd(&counters[0], 1u);
            out[slot] = LoopCandidate{dist, (int64_t)d};
        }
    }
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&counters[1], 1u) == gridDim.x - 1) { // the last workgroup: every append is in
            __threadfence();
            *out_n = (int64_t)atomicAdd(&counters[0], 0u);
            counters[0] = 0;
            counters[1] = 0;
        }
    }
}

// k_loop_candidates with the argmin kept: same launch, same counters, same order of events; out holds
// LoopCandidateShift records.
__global__ __launch_bounds__(64) void k_loop_candidates_shift(const double *__restrict__ table, const int32_t *__restrict__ labels,
                                                              int32_t q, int32_t frame_gap, double threshold,
                                                              unsigned *__restrict__ counters, LoopCandidateShift *out,
                                                              int64_t *out_n)
{
    const int32_t d = blockIdx.x;
    if ((int64_t)labels[q] - (int64_t)labels[d] >= (int64_t)frame_gap) {
        int shift;
        const double dist = sc_distance_shift(table + (size_t)q * kScCells, table + (size_t)d * kScCells, shift);
        if (threadIdx.x == 0 && dist < threshold) { // strict; NaN never passes
            const unsigned slot = atomicAdd(&counters[0], 1u);
            out[slot] = LoopCandidateShift{dist, d, shift};
        }
    }
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&counters[1], 1u) == gridDim.x - 1) { // the last workgroup: every append is in
            __threadfence();
            *out_n = (int64_t)atomicAdd(&counters[0], 0u);
            counters[0] = 0;
            counters[1] = 0;
        }
    }
}

} // namespace icpmi
