// static_map.h -- the map's point products without the rows the counts outvote (not in the reference).
// The count plane (raycount.h, live_counts.h) knows which cells held something that later went away; k_map_world
// (global_map.h) moves every row of every kept scan into the world all the same, so whatever moved while the node drove
// is smeared along its path.  Here every row of the used frames gets a label against the live plane, and the world
// points of the rows that are kept are written in frame then row order: a stable compaction, so the output is
// byte-comparable and the voxel filter behind it sums each centroid in the order it would on the host.
//
// The contract (include/icp_mi355x.h and scripts/static_map_ref.py state it in the same words), with hits[c], misses[c]
// and probability[c] exactly what icpmi_map_raycast_counts defines for the used frames and the caller's grid:
//   A row of used frame i VOTES iff it marks a cell c under the rules the counts use: grid_cell_key of its world
//   point with frame i's translation as the sensor and, while icpmi_map_set_ground is on, additionally its label is
//   OBSTACLE and the band is open.  With n = hits[c] + misses[c] a row's label is
//     0  kept, does not vote: ground rows, rows out of band or ring, non-finite rows, an unrepresentable quotient
//     1  kept, votes
//     2  dropped: the row votes, n >= rule.min_observations and probability[c] < rule.min_probability
//   probability[c] = (200 hits[c] + n) / (2 n) in integer division.  A lookup that finds n == 0, or a cell outside
//   the plane's box, keeps the row with label 1 (it cannot happen for a voting row).  min_probability == 0 drops
//   nothing.  All integer: no dependence on the order of frames, rows or threads.
//
//     k_static_label   one workgroup of 256 per MapTile, four rows per thread, the pose through scalar loads
//                      (k_map_world's shape): world point, key, ground mask, one word of the plane, the label byte; per
//                      tile its kept, voting and dropped rows from 64-bit wave ballots, the four waves through LDS
//     (exclusive sum)  of the tiles' kept rows (rocPRIM, sort.hip)
//     k_static_world   the same world point again; a kept row's rank within its tile, in row order, is the kept rows
//                      of the sweeps before its own, of the waves before its own in its sweep, and of the lanes below
//                      it in its wave (mbcnt over the ballot); it is written at tile offset + rank
// Two HBM streams: 24 B + 1 B read and 1 B written per row, then 24 B + 1 B read and 24 B written per kept row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.h"
#include "global_map.h"
#include "ground.h"
#include "occupancy.h"
#include "raycount.h"

namespace icpmi {

constexpr uint8_t kStaticQuiet = 0, kStaticVotes = 1, kStaticDropped = 2;
constexpr int kStaticSweeps = kMapTileRows / 256; // a thread's rows: r = threadIdx.x + 256 b
static_assert(kStaticSweeps == 4, "four rows per thread");

struct StaticPlane {     // the live plane: cells [x0, x0 + w) x [y0, y0 + h), one word each (w == 0: no plane)
    const unsigned *words;
    long long x0, y0, w, h;
};

struct StaticRuleK {     // icpmi_static_rule, validated
    int32_t min_probability, min_observations;
};

struct StaticTotals {    // over the tiles of one k_static_label launch
    unsigned long long voting, dropped;
};

// The label of a row whose key is `key` (kGridNone: it marks nothing).
__device__ __forceinline__ uint8_t static_label_of(unsigned long long key, const StaticPlane &pl, const StaticRuleK &rule)
{
    if (key == kGridNone) return kStaticQuiet;
    const long long lx = (long long)(int)((unsigned)(key >> 32) ^ 0x80000000u) - pl.x0;
    const long long ly = (long long)(int)((unsigned)key ^ 0x80000000u) - pl.y0;
    if (lx < 0 || ly < 0 || lx >= pl.w || ly >= pl.h) return kStaticVotes;
    const unsigned v = pl.words[(size_t)ly * (size_t)pl.w + (size_t)lx];
    const unsigned hits = v >> 16, n = hits + (v & 0xffffu);
    if (n == 0u || (long long)n < (long long)rule.min_observations) return kStaticVotes;
    return count_probability(hits, v & 0xffffu) < rule.min_probability ? kStaticDropped : kStaticVotes;
}

// tiles: the launch's tiles (one workgroup each); poses: 16 doubles per frame from frame 0 on; ground: one label per
// store row, or null (then g carries the band; with ground the caller opens it); labels: one byte per store row;
// kept: per tile of the launch its kept rows; totals: zero before the launch.
__global__ __launch_bounds__(256) void k_static_label(const double *__restrict__ store, const MapTile *__restrict__ tiles,
                                                      const double *__restrict__ poses, const uint8_t *__restrict__ ground,
                                                      StaticPlane pl, GridParams g, StaticRuleK rule,
                                                      uint8_t *__restrict__ labels, unsigned *__restrict__ kept,
                                                      StaticTotals *__restrict__ totals)
{
    constexpr int B = kStaticSweeps;
    __shared__ unsigned part[2][4];
    const MapTile t = tiles[blockIdx.x];
    const Rigid34 P = Rigid34::load(poses + 16 * (size_t)t.frame);
    const double *in = store + 3 * (size_t)t.row0;
    double x[B], y[B], z[B];
#pragma unroll
    for (int b = 0; b < B; ++b) { // every load of the thread first
        const int r = (int)threadIdx.x + 256 * b;
        x[b] = y[b] = z[b] = 0.0;
        if (r < t.rows) x[b] = in[3 * r], y[b] = in[3 * r + 1], z[b] = in[3 * r + 2];
    }
    unsigned voting = 0u, dropped = 0u; // wave-uniform
#pragma unroll
    for (int b = 0; b < B; ++b) {   // (no early exit: every lane takes part in the ballots)
        const int r = (int)threadIdx.x + 256 * b;
        const bool valid = r < t.rows;
        uint8_t label = kStaticQuiet;
        if (valid) {
            double px, py, pz;
            P.apply(x[b], y[b], z[b], px, py, pz);
            unsigned long long key = grid_cell_key(px, py, pz, g, P.t0, P.t1);
            if (ground && ground[(size_t)t.row0 + (size_t)r] != kGroundObstacle) key = kGridNone;
            label = static_label_of(key, pl, rule);
            labels[(size_t)t.row0 + (size_t)r] = label;
        }
        voting += (unsigned)__popcll(__ballot(label != kStaticQuiet));
        dropped += (unsigned)__popcll(__ballot(label == kStaticDropped));
    }
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    if (lane == 0) part[0][wave] = voting, part[1][wave] = dropped;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned v = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
        const unsigned d = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
        kept[blockIdx.x] = (unsigned)t.rows - d;
        if (v) atomicAdd(&totals->voting, (unsigned long long)v);
        if (d) atomicAdd(&totals->dropped, (unsigned long long)d);
    }
}

// tiles, poses, labels: k_static_label's; offsets: per tile of the launch the kept rows of the tiles before it, counted
// from tile 0 of the scan they come from; base: that count at the launch's first tile; world: the kept rows' world
// points, row 0 being the first kept row of the launch's first tile.
__global__ __launch_bounds__(256) void k_static_world(const double *__restrict__ store, const MapTile *__restrict__ tiles,
                                                      const double *__restrict__ poses, const uint8_t *__restrict__ labels,
                                                      const unsigned *__restrict__ offsets, unsigned base,
                                                      double *__restrict__ world)
{
    constexpr int B = kStaticSweeps;
    __shared__ unsigned part[B][4];
    const MapTile t = tiles[blockIdx.x];
    const Rigid34 P = Rigid34::load(poses + 16 * (size_t)t.frame);
    const double *in = store + 3 * (size_t)t.row0;
    const uint8_t *lab = labels + (size_t)t.row0;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    double x[B], y[B], z[B];
    bool keep[B];
#pragma unroll
    for (int b = 0; b < B; ++b) { // every load of the thread first
        const int r = (int)threadIdx.x + 256 * b;
        x[b] = y[b] = z[b] = 0.0;
        keep[b] = false;
        if (r < t.rows) x[b] = in[3 * r], y[b] = in[3 * r + 1], z[b] = in[3 * r + 2], keep[b] = lab[r] != kStaticDropped;
    }
    unsigned below[B]; // the kept rows in the lanes below this one, per sweep
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const unsigned long long m = __ballot(keep[b]);
        below[b] = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (lane == 0) part[b][wave] = (unsigned)__popcll(m);
    }
    __syncthreads();
    const size_t o0 = (size_t)(offsets[blockIdx.x] - base);
    unsigned before = 0u; // the kept rows of the sweeps before b
#pragma unroll
    for (int b = 0; b < B; ++b) {
        unsigned rank = before + below[b];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) rank += part[b][w];
            before += part[b][w];
        }
        if (keep[b]) {
            double px, py, pz;
            P.apply(x[b], y[b], z[b], px, py, pz);
            const size_t o = o0 + (size_t)rank;
            world[3 * o] = px;
            world[3 * o + 1] = py;
            world[3 * o + 2] = pz;
        }
    }
}

} // namespace icpmi
