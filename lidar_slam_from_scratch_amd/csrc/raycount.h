// raycount.h -- the kept scans ray-cast into per-cell hit and miss counts.  raycast.h's raster lets one
// return block a cell for good ("occupied wins" over every frame); here a cell records how many used frames saw it
// occupied and how many saw through it.  The frames, hit cells, sensor cells and walk are raycast.h's.  For a used
// frame i, H_i is the set of its distinct hit cells and C_i the cells carved by any of its rays, less H_i (within one
// scan occupied wins); hits[c] = #{i : c in H_i}, misses[c] = #{i : c in C_i}: a frame adds at most 1 to each.
//     k_ray_count<true>   one workgroup per frame: two bit windows (carved, hit) of (2R + 3)^2 cells in LDS; after the
//                         walk, one atomic add per (cell, frame) into the count plane
//     k_ray_count<false>  the same body with the windows in device scratch (a pair too large for LDS): a fixed
//                         number of persistent workgroups, each owning one pair and taking every gridDim.x-th frame
//     k_count_bounds      tight bounds of the observed cells, their number, the hit cells' number and the two maxima,
//                         one pass over the count plane
//     k_count_raster      the cropped hits, misses (uint16) and probability (int8) arrays
// The count plane holds one 32-bit word per plane cell: hits in the high half, misses in the low.  A call uses at most
// 65,535 frames, so neither half can carry.  Integer adds throughout: the results do not depend on the order of
// frames, rows or threads.  scripts/map_ref.py's MapRef.raycast_counts restates the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "raycast.h"

namespace icpmi {

constexpr int kCountMaxFrames = 65535;    // ICPMI_RAYCOUNT_MAX_FRAMES: a count is 16 bits and a frame adds at most 1
constexpr int kCountLdsMaxR = 392;        // ICPMI_RAYCOUNT_LDS_MAX_R: the largest pair of windows within kRayLdsBytes
constexpr int kCountLdsPlainMaxR = 239;   // ... and within the 64 KiB a launch gets without asking
constexpr size_t kCountScratchBytes = (size_t)256 << 20;   // k_ray_count<false>'s windows, all workgroups together
constexpr int kCountScratchGroups = 256;  // ... and at most one workgroup per CU
static_assert(8 * ray_window_words(kCountLdsMaxR) <= kRayLdsBytes && 8 * ray_window_words(kCountLdsMaxR + 1) > kRayLdsBytes,
              "kCountLdsMaxR is the largest R whose two windows fit");
static_assert(8 * ray_window_words(kCountLdsPlainMaxR) <= 64 * 1024 && 8 * ray_window_words(kCountLdsPlainMaxR + 1) > 64 * 1024,
              "kCountLdsPlainMaxR is the largest R whose two windows fit 64 KiB");
static_assert(8 * (size_t)ray_window_words(kRayMaxR) <= kCountScratchBytes, "the budget holds one pair at the largest R");

constexpr unsigned kCountHit = 1u << 16, kCountMiss = 1u;

struct CountBounds {  // in plane coordinates; max < 0: no observed cell
    int32_t min_x, min_y, max_x, max_y;
    unsigned long long n_observed, n_hit_cells;
    int32_t max_hits, max_misses;
};
static_assert(sizeof(CountBounds) == 40, "copied to the host as it is");

// The workgroups k_ray_count<false> runs with: what the scratch budget holds, no more than there are frames.
inline int count_scratch_groups(int R, int64_t frames)
{
    const size_t pair = 8 * (size_t)ray_window_words(R);
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(kCountScratchGroups, frames), (int64_t)(kCountScratchBytes / pair)));
}

// keys: k_map_world's, indexed by store row.  counts: pl.w * pl.h words, row-major, zero before the launch.
// kLds: gridDim.x == n_frames, dynamic LDS of 2 * ray_window_words(R) words, scratch unused.  Otherwise scratch holds
// gridDim.x pairs of windows, zero before the launch and zero again after it.
template <bool kLds>
__global__ __launch_bounds__(kRayThreads) void k_ray_count(const unsigned long long *__restrict__ keys,
                                                           const RayFrame *__restrict__ frames, int n_frames, int R, RayPlane pl,
                                                           unsigned *__restrict__ scratch, unsigned *__restrict__ counts)
{
    extern __shared__ unsigned count_window[];
    const int side = 2 * R + 3, wwpr = ray_window_row_words(R), words = side * wwpr;
    unsigned *const carvedw = kLds ? count_window : scratch + (size_t)blockIdx.x * 2 * (size_t)words;
    unsigned *const hitw = carvedw + words;
    auto set = [](unsigned *w, unsigned bit) {
        if constexpr (kLds) ray_set_lds(w, bit);
        else ray_set_global(w, bit);    // agent-scope, relaxed: the window is this workgroup's alone
    };
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    for (int fi = (int)blockIdx.x; fi < n_frames; fi += (int)gridDim.x) {
        const RayFrame f = frames[fi];
        if (f.rows == 0) continue;
        const int wx0 = f.sx - (R + 1) - pl.x0, wy0 = f.sy - (R + 1) - pl.y0; // the window's corner in the plane, >= 0
        const int word0 = wx0 >> 5, cx = (wx0 & 31) + R + 1, cy = R + 1;      // the sensor cell in the window
        if constexpr (kLds) {
            for (int i = (int)threadIdx.x; i < 2 * words; i += kRayThreads) count_window[i] = 0u;
            __syncthreads();
        }
        for (int r = (int)threadIdx.x; r < f.rows; r += kRayThreads) {
            int ddx, ddy;
            if (!ray_hit(keys[f.row0 + r], f, R, ddx, ddy)) continue;
            const int hx = cx + ddx, hy = cy + ddy;
            set(hitw + hy * wwpr + (hx >> 5), 1u << (hx & 31));
            ray_walk(cx, cy, hx, hy, [&](int x, int y) { set(carvedw + y * wwpr + (x >> 5), 1u << (x & 31)); });
        }
        if constexpr (!kLds) __threadfence();
        __syncthreads();
        // the flush: a wave takes two window words as 64 cells, lane l the cell of bit l & 31 of word 2p + (l >> 5),
        // so that its adds fall on consecutive words of the count plane
        for (int p = wave; 2 * p < words; p += kRayThreads / 64) {
            const int i = 2 * p + (lane >> 5);
            unsigned h = 0u, c = 0u;
            if (i < words) {
                if constexpr (kLds) h = hitw[i], c = carvedw[i] & ~h;
                else {
                    h = __hip_atomic_load(hitw + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    c = __hip_atomic_load(carvedw + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ~h;
                }
            }
            if (!__any((h | c) != 0u)) continue;
            if constexpr (!kLds) {  // left clear for the workgroup's next frame
                if ((lane & 31) == 0 && i < words) {
                    __hip_atomic_store(hitw + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(carvedw + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            const unsigned bit = 1u << (lane & 31);
            const unsigned add = (h & bit) ? kCountHit : ((c & bit) ? kCountMiss : 0u);
            const int row = i / wwpr, j = i - row * wwpr;
            const int x = 32 * (word0 + j) + (lane & 31), y = wy0 + row;
            if (add != 0u && x < pl.w && y < pl.h)
                (void)__hip_atomic_fetch_add(counts + (size_t)y * (size_t)pl.w + (size_t)x, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if constexpr (!kLds) {
            __threadfence();
            __syncthreads();
        }
    }
}

// out: {INT_MAX, INT_MAX, -1, -1, 0, 0, 0, 0} before the launch.  A workgroup takes whole plane rows.
__global__ __launch_bounds__(256) void k_count_bounds(const unsigned *__restrict__ counts, RayPlane pl, CountBounds *__restrict__ out)
{
    int min_x = INT32_MAX, min_y = INT32_MAX, max_x = -1, max_y = -1, max_h = 0, max_m = 0;
    unsigned long long n_obs = 0, n_hit = 0;
    for (int y = (int)blockIdx.x; y < pl.h; y += (int)gridDim.x) {
        const unsigned *row = counts + (size_t)y * (size_t)pl.w;
        for (int x = (int)threadIdx.x; x < pl.w; x += 256) {
            const unsigned v = row[x];
            if (v == 0u) continue;
            min_x = min(min_x, x), max_x = max(max_x, x);
            min_y = min(min_y, y), max_y = max(max_y, y);
            max_h = max(max_h, (int)(v >> 16)), max_m = max(max_m, (int)(v & 0xffffu));
            n_obs += 1;
            n_hit += (v >> 16) != 0u;
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
    __shared__ int part[4][6];
    __shared__ unsigned long long part_n[4][2];
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = min_x, part[wave][1] = min_y, part[wave][2] = max_x, part[wave][3] = max_y;
        part[wave][4] = max_h, part[wave][5] = max_m;
        part_n[wave][0] = n_obs, part_n[wave][1] = n_hit;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) {
        min_x = min(min_x, part[w][0]), min_y = min(min_y, part[w][1]);
        max_x = max(max_x, part[w][2]), max_y = max(max_y, part[w][3]);
        max_h = max(max_h, part[w][4]), max_m = max(max_m, part[w][5]);
        n_obs += part_n[w][0], n_hit += part_n[w][1];
    }
    if (max_x < 0) return; // nothing observed in this workgroup's rows
    atomicMin(&out->min_x, min_x);
    atomicMin(&out->min_y, min_y);
    atomicMax(&out->max_x, max_x);
    atomicMax(&out->max_y, max_y);
    atomicMax(&out->max_hits, max_h);
    atomicMax(&out->max_misses, max_m);
    atomicAdd(&out->n_observed, n_obs);
    atomicAdd(&out->n_hit_cells, n_hit);
}

// 100 * hits / n rounded half up, n = hits + misses > 0: the counting model, in integers
__device__ __forceinline__ int count_probability(unsigned hits, unsigned misses)
{
    const unsigned n = hits + misses;
    return (int)((200u * hits + n) / (2u * n));
}

// raster cell (i, j) is plane cell (bx + i, by + j); the raster's margin may reach past the plane
__global__ __launch_bounds__(256) void k_count_raster(const unsigned *__restrict__ counts, RayPlane pl, int bx, int by, int width,
                                                      int height, uint16_t *__restrict__ hits, uint16_t *__restrict__ misses,
                                                      int8_t *__restrict__ probability)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)width * (size_t)height) return;
    const int j = (int)(idx / (size_t)width), i = (int)(idx - (size_t)j * (size_t)width);
    const int x = bx + i, y = by + j;
    unsigned v = 0u;
    if (x >= 0 && x < pl.w && y >= 0 && y < pl.h) v = counts[(size_t)y * (size_t)pl.w + (size_t)x];
    hits[idx] = (uint16_t)(v >> 16);
    misses[idx] = (uint16_t)(v & 0xffffu);
    probability[idx] = v == 0u ? (int8_t)-1 : (int8_t)count_probability(v >> 16, v & 0xffffu);
}

} // namespace icpmi
