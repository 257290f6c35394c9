// live_counts.h -- the hit / miss counts kept while the node drives.  raycount.h builds the count plane
// of every kept scan at once, one workgroup per frame; here the plane persists in the handle and a call casts only the
// frames that are new, so one frame has to be spread over the chip instead.  The count word, the window layout, the
// hit test and the walk are raycount.h's and raycast.h's; the result is the batch's byte for byte, integer sums
// being independent of order.  Per new frame, two launches:
//     k_live_carve   up to kLiveGroups workgroups share the frame's rows; each walks its share into its own pair of
//                    bit windows (carved, hit) in LDS, as k_ray_count<true> does, and then ORs the non-zero words into
//                    one frame-sized pair of windows in device memory (zero between frames)
//     k_live_apply   over the device windows: h = hit, c = carved & ~hit ("within one scan occupied wins" needs every
//                    hit of the frame before any miss is added: the kernel boundary gives that); lanes take
//                    consecutive cells and add to the plane with a plain load, add and store (frames are serialised
//                    on the stream and a cell has one owner); the window words read are cleared; and the running
//                    CountBounds is updated from each word before and after its add
// and, when a frame's window leaves the plane's box (live_plane.h):
//     k_plane_move   the old plane's words into the new, larger, zeroed one, and the running bounds with them
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "raycount.h"

namespace icpmi {

#ifndef ICPMI_LIVE_GROUPS          // scripts/live_timing.py builds the values it compares; see profiles/live/tried.txt
#define ICPMI_LIVE_GROUPS 16
#endif
#ifndef ICPMI_LIVE_BATCH_FRAMES
#define ICPMI_LIVE_BATCH_FRAMES 8
#endif
constexpr int kLiveGroups = ICPMI_LIVE_GROUPS;            // the most workgroups one frame's rows are shared among
constexpr int kLiveGroupRows = kRayThreads;               // ... and the fewest rows worth a workgroup of its own
constexpr int kLiveBatchFrames = ICPMI_LIVE_BATCH_FRAMES; // more pending frames than this go through k_ray_count
constexpr int kLiveApplyThreads = 256, kLiveApplyGroups = 128;

// The workgroups a frame of `rows` rows (> 0) is carved by, and the rows each takes (the last one fewer).
inline int live_carve_groups(int rows) { return std::max(1, std::min(kLiveGroups, (rows + kLiveGroupRows - 1) / kLiveGroupRows)); }
inline int live_carve_share(int rows) { const int g = live_carve_groups(rows); return (rows + g - 1) / g; }

// keys: k_map_world's for the call's new frames, f.row0 counted from the first of them.  shift: the bit of the
// window's first column in its first word (the window's corner in the plane, & 31).  win: 2 * ray_window_words(R)
// words, carved then hit, zero before the frame's first launch.  Dynamic LDS: as many words.
__global__ __launch_bounds__(kRayThreads) void k_live_carve(const unsigned long long *__restrict__ keys, RayFrame f, int R, int shift,
                                                            int share, unsigned *__restrict__ win)
{
    extern __shared__ unsigned live_lds[];
    const int r0 = (int)blockIdx.x * share, r1 = min(f.rows, r0 + share);
    if (r0 >= r1) return;
    const int side = 2 * R + 3, wwpr = ray_window_row_words(R), words = side * wwpr;
    unsigned *const carvedw = live_lds, *const hitw = live_lds + words;
    const int cx = shift + R + 1, cy = R + 1; // the sensor cell in the window
    for (int i = (int)threadIdx.x; i < 2 * words; i += kRayThreads) live_lds[i] = 0u;
    __syncthreads();
    for (int r = r0 + (int)threadIdx.x; r < r1; r += kRayThreads) {
        int ddx, ddy;
        if (!ray_hit(keys[f.row0 + r], f, R, ddx, ddy)) continue;
        const int hx = cx + ddx, hy = cy + ddy;
        ray_set_lds(hitw + hy * wwpr + (hx >> 5), 1u << (hx & 31));
        ray_walk(cx, cy, hx, hy, [&](int x, int y) { ray_set_lds(carvedw + y * wwpr + (x >> 5), 1u << (x & 31)); });
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < 2 * words; i += kRayThreads) {
        const unsigned v = live_lds[i];
        if (v != 0u) ray_set_global(win + i, v);
    }
}

// (wx0, wy0): the window's corner in the plane, >= 0.  A wave takes two window words as 64 cells, lane l the cell of
// bit l & 31 of word 2p + (l >> 5), as k_ray_count's flush does.  bounds: the plane's running CountBounds.
__global__ __launch_bounds__(kLiveApplyThreads) void k_live_apply(unsigned *__restrict__ win, int R, int wx0, int wy0, RayPlane pl,
                                                                  unsigned *__restrict__ plane, CountBounds *__restrict__ bounds)
{
    const int side = 2 * R + 3, wwpr = ray_window_row_words(R), words = side * wwpr;
    const int word0 = wx0 >> 5;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    constexpr int kWaves = kLiveApplyThreads / 64;
    int min_x = INT32_MAX, min_y = INT32_MAX, max_x = -1, max_y = -1, max_h = 0, max_m = 0;
    unsigned n_obs = 0, n_hit = 0;
    for (int p = (int)blockIdx.x * kWaves + wave; 2 * p < words; p += (int)gridDim.x * kWaves) {
        const int i = 2 * p + (lane >> 5);
        unsigned h = 0u, c = 0u;
        if (i < words) {
            h = __hip_atomic_load(win + words + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            c = __hip_atomic_load(win + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ~h;
        }
        if (!__any((h | c) != 0u)) continue;
        if ((lane & 31) == 0 && i < words) { // left clear for the next frame
            __hip_atomic_store(win + words + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(win + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const unsigned bit = 1u << (lane & 31);
        const unsigned add = (h & bit) ? kCountHit : ((c & bit) ? kCountMiss : 0u);
        const int row = i / wwpr, j = i - row * wwpr;
        const int x = 32 * (word0 + j) + (lane & 31), y = wy0 + row;
        if (add != 0u && x < pl.w && y < pl.h) {
            unsigned *const cell = plane + (size_t)y * (size_t)pl.w + (size_t)x;
            const unsigned before = *cell, after = before + add;
            *cell = after;
            min_x = min(min_x, x), max_x = max(max_x, x);
            min_y = min(min_y, y), max_y = max(max_y, y);
            max_h = max(max_h, (int)(after >> 16)), max_m = max(max_m, (int)(after & 0xffffu));
            n_obs += before == 0u;
            n_hit += (before >> 16) == 0u && add == kCountHit;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        min_x = min(min_x, __shfl_down(min_x, d));
        min_y = min(min_y, __shfl_down(min_y, d));
        max_x = max(max_x, __shfl_down(max_x, d));
        max_y = max(max_y, __shfl_down(max_y, d));
        max_h = max(max_h, __shfl_down(max_h, d));
        max_m = max(max_m, __shfl_down(max_m, d));
        n_obs += __shfl_down(n_obs, d);
        n_hit += __shfl_down(n_hit, d);
    }
    __shared__ int part[kWaves][6];
    __shared__ unsigned part_n[kWaves][2];
    if (lane == 0) {
        part[wave][0] = min_x, part[wave][1] = min_y, part[wave][2] = max_x, part[wave][3] = max_y;
        part[wave][4] = max_h, part[wave][5] = max_m;
        part_n[wave][0] = n_obs, part_n[wave][1] = n_hit;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kWaves; ++w) {
        min_x = min(min_x, part[w][0]), min_y = min(min_y, part[w][1]);
        max_x = max(max_x, part[w][2]), max_y = max(max_y, part[w][3]);
        max_h = max(max_h, part[w][4]), max_m = max(max_m, part[w][5]);
        n_obs += part_n[w][0], n_hit += part_n[w][1];
    }
    if (max_x < 0) return; // this workgroup added nothing
    // tested first: after the first frames few adds move a bound, and an atomic leaves L2
    auto load = [](const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    if (min_x < load(&bounds->min_x)) atomicMin(&bounds->min_x, min_x);
    if (min_y < load(&bounds->min_y)) atomicMin(&bounds->min_y, min_y);
    if (max_x > load(&bounds->max_x)) atomicMax(&bounds->max_x, max_x);
    if (max_y > load(&bounds->max_y)) atomicMax(&bounds->max_y, max_y);
    if (max_h > load(&bounds->max_hits)) atomicMax(&bounds->max_hits, max_h);
    if (max_m > load(&bounds->max_misses)) atomicMax(&bounds->max_misses, max_m);
    if (n_obs) atomicAdd(&bounds->n_observed, (unsigned long long)n_obs);
    if (n_hit) atomicAdd(&bounds->n_hit_cells, (unsigned long long)n_hit);
}

// src: ow x oh words; dst: nw words per row, zero before the launch; the old plane's cell (x, y) becomes (x + dx,
// y + dy), dx, dy >= 0.  A workgroup takes whole rows.  The running bounds move with the cells.
__global__ __launch_bounds__(256) void k_plane_move(const unsigned *__restrict__ src, int ow, int oh, unsigned *__restrict__ dst, int nw,
                                                    int dx, int dy, CountBounds *__restrict__ bounds)
{
    for (int y = (int)blockIdx.x; y < oh; y += (int)gridDim.x) {
        const unsigned *from = src + (size_t)y * (size_t)ow;
        unsigned *to = dst + (size_t)(y + dy) * (size_t)nw + (size_t)dx;
        for (int x = (int)threadIdx.x; x < ow; x += 256) to[x] = from[x];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && bounds->max_x >= 0) {
        bounds->min_x += dx, bounds->max_x += dx;
        bounds->min_y += dy, bounds->max_y += dy;
    }
}

} // namespace icpmi
