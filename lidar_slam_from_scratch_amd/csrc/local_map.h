// local_map.h -- the sliding voxel map of scan-to-local-map odometry (the target of LOAM / KISS-ICP style front ends;
// not in the reference node, which registers each scan against the one before it, slam_node.cpp:132-138).
// The table: sorted unique 63-bit voxel keys and one fp64 point per key, double-buffered (icpmi_local_map, capi.hip).
// One add(scan, pose) evicts the residents out of range of the pose, inserts the lowest scan row of every voxel that
// no surviving resident holds, and writes survivors and insertions, merged by key, into the other buffer:
//     k_lmap_keys      per scan row: world point (Rigid34::apply), absolute key, dropped rows counted
//     sort_pairs_u64_all   stable, all 64 bits: (key, row); a dropped row's key is kLmapDropped and sorts behind every key
//     k_lmap_marks     residents: the range test; sorted rows: head of run, not dropped, key not among the surviving residents
//     exclusive_sum_u32    over both mark arrays at once (and one closing zero: the totals)
//     k_lmap_merge     each kept element to its own rank + the kept elements of the other list below its key
// Ten kernel launches for an 8.5k-row scan (the sort is five of them, the sum two).  Every kernel is a
// grid-stride loop of 256-thread workgroups, at most kLmapMaxBlocks of them.  HBM streams: 24 B read + 36 B written per scan row by the keys, 32 B per
// resident and 12 B per row by the marks (plus the searches' log2 probes, which hit L2), 32 B written per kept element.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "device_math.h"

namespace icpmi {

constexpr int kLmapMaxBlocks = 2048;                        // 256 CUs x 8 workgroups
constexpr unsigned long long kLmapDropped = ~0ull;          // bit 63 set: no key has it
constexpr double kLmapCellLimit = 1048576.0;                // cells [-2^20, 2^20) per axis
constexpr int kLmapS = 0, kLmapTotal = 1, kLmapDroppedRows = 2; // the words an add reads back

inline int lmap_blocks(size_t work) { return (int)std::max<size_t>(1, std::min<size_t>((work + 255) / 256, kLmapMaxBlocks)); }

// d2 <= r2 against the pose's translation; a NaN fails
__device__ __forceinline__ bool lmap_in_range(double px, double py, double pz, double tx, double ty, double tz, double r2)
{
    const double dx = px - tx, dy = py - ty, dz = pz - tz;
    return (dx * dx + dy * dy) + dz * dz <= r2;
}

// first index in [0, n) whose key is not below k (n: none)
__device__ __forceinline__ unsigned lmap_lower_bound(const unsigned long long *__restrict__ keys, unsigned n, unsigned long long k)
{
    unsigned lo = 0, hi = n;
    while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Per scan row: the world point, and its key -- floor(p / voxel) per axis, accepted in [-2^20, 2^20) (the comparison is
// made on the double, so an infinite or NaN coordinate fails it before any cast), offset by 2^20, 21 bits each -- or
// kLmapDropped when a cell is outside that, or the point is out of range of the pose.  vals[i] = i.
__global__ __launch_bounds__(256) void k_lmap_keys(const double *__restrict__ scan, unsigned n, Rigid34 P, double voxel, double r2,
                                                   double *__restrict__ world, unsigned long long *__restrict__ keys,
                                                   unsigned *__restrict__ vals, unsigned *__restrict__ words)
{
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        double px, py, pz;
        P.apply(scan[3 * (size_t)i], scan[3 * (size_t)i + 1], scan[3 * (size_t)i + 2], px, py, pz);
        world[3 * (size_t)i] = px;
        world[3 * (size_t)i + 1] = py;
        world[3 * (size_t)i + 2] = pz;
        const double fx = floor(px / voxel), fy = floor(py / voxel), fz = floor(pz / voxel);
        const bool cells = fx >= -kLmapCellLimit && fx < kLmapCellLimit && fy >= -kLmapCellLimit && fy < kLmapCellLimit &&
                           fz >= -kLmapCellLimit && fz < kLmapCellLimit;
        unsigned long long key = kLmapDropped;
        if (cells && lmap_in_range(px, py, pz, P.t0, P.t1, P.t2, r2)) {
            const unsigned long long cx = (unsigned long long)((long long)fx + 1048576), cy = (unsigned long long)((long long)fy + 1048576),
                                     cz = (unsigned long long)((long long)fz + 1048576);
            key = (cx << 42) | (cy << 21) | cz;
        } else {
            atomicAdd(words + kLmapDroppedRows, 1u); // (one add per wave of the lanes that take this branch)
        }
        keys[i] = key;
        vals[i] = i;
    }
}

// marks[0, R): the resident is in range of the pose.  marks[R + j], j in [0, n): sorted row j is inserted -- not dropped,
// the first of its key's run (the sort is stable: the lowest scan row), and its key is not a surviving resident's (an
// evicted resident's voxel is taken again by this scan's row).  marks[R + n] = 0, so that the sum's last entry is the total.
__global__ __launch_bounds__(256) void k_lmap_marks(const unsigned long long *__restrict__ res_keys, const double *__restrict__ res_pts,
                                                    unsigned R, const unsigned long long *__restrict__ new_keys, unsigned n,
                                                    double tx, double ty, double tz, double r2, unsigned *__restrict__ marks)
{
    const size_t total = (size_t)R + n + 1;
    for (size_t e = blockIdx.x * 256u + threadIdx.x; e < total; e += (size_t)gridDim.x * 256u) {
        unsigned mark = 0;
        if (e < R) {
            mark = lmap_in_range(res_pts[3 * e], res_pts[3 * e + 1], res_pts[3 * e + 2], tx, ty, tz, r2);
        } else if (e < (size_t)R + n) {
            const unsigned j = (unsigned)(e - R);
            const unsigned long long k = new_keys[j];
            if (k != kLmapDropped && (j == 0 || new_keys[j - 1] != k)) {
                const unsigned p = lmap_lower_bound(res_keys, R, k);
                const bool held = p < R && res_keys[p] == k &&
                                  lmap_in_range(res_pts[3 * (size_t)p], res_pts[3 * (size_t)p + 1], res_pts[3 * (size_t)p + 2], tx, ty, tz, r2);
                mark = !held;
            }
        }
        marks[e] = mark;
    }
}

// offs: the exclusive sum of marks (R + n + 1 entries): offs[R] = surviving residents S, offs[R + n] = rows of the new
// table.  A kept resident i goes to offs[i] + (kept rows below its key); a kept row j to (offs[R + j] - S) + (kept
// residents below its key).  Nothing is written when the new table would not fit (the add then fails and the old
// buffer stays the table).  words[kLmapS], words[kLmapTotal] receive the two counts.
__global__ __launch_bounds__(256) void k_lmap_merge(const unsigned long long *__restrict__ res_keys, const double *__restrict__ res_pts,
                                                    unsigned R, const unsigned long long *__restrict__ new_keys,
                                                    const unsigned *__restrict__ new_rows, const double *__restrict__ world, unsigned n,
                                                    const unsigned *__restrict__ marks, const unsigned *__restrict__ offs,
                                                    unsigned long long capacity, unsigned long long *__restrict__ out_keys,
                                                    double *__restrict__ out_pts, unsigned *__restrict__ words)
{
    const unsigned S = offs[R], rows = offs[(size_t)R + n];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        words[kLmapS] = S;
        words[kLmapTotal] = rows;
    }
    if ((unsigned long long)rows > capacity) return;
    const size_t total = (size_t)R + n;
    for (size_t e = blockIdx.x * 256u + threadIdx.x; e < total; e += (size_t)gridDim.x * 256u) {
        if (!marks[e]) continue;
        unsigned long long key;
        const double *p;
        size_t slot;
        if (e < R) {
            key = res_keys[e];
            p = res_pts + 3 * e;
            slot = (size_t)offs[e] + (offs[(size_t)R + lmap_lower_bound(new_keys, n, key)] - S);
        } else {
            const unsigned j = (unsigned)(e - R);
            key = new_keys[j];
            p = world + 3 * (size_t)new_rows[j];
            slot = (size_t)(offs[e] - S) + offs[lmap_lower_bound(res_keys, R, key)];
        }
        out_keys[slot] = key;
        out_pts[3 * slot] = p[0];
        out_pts[3 * slot + 1] = p[1];
        out_pts[3 * slot + 2] = p[2];
    }
}

} // namespace icpmi
