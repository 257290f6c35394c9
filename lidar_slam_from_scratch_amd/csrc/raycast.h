// raycast.h -- the kept scans ray-cast into a free / occupied / unknown raster.  The reference's
// cells_to_occupancy_grid_msg (slam_viz/src/ros/slam_node.cpp:279-297) writes 100 for a hit cell and 0 everywhere else,
// so space the LiDAR never saw is published as free.  Here every hit of every used frame (k_map_world's keys:
// grid_cell_key under the frame's own sensor position) marks its cell occupied and carves the cells of the all-integer
// Bresenham line from the frame's sensor cell to it: the sensor cell is carved, the hit cell is not.
//     k_ray_carve_lds     one workgroup per frame; the frame's rays are walked in a bit window of (2R + 3)^2 cells
//                         centred on its sensor cell in LDS, whose non-zero words are then ORed into the global plane
//     k_ray_carve_global  one workgroup per tile of the tile table; the walk ORs straight into the global plane (a
//                         window too large for LDS)
//     k_ray_bounds        tight bounds of occupied | carved and the two counts, one pass over both planes
//     k_ray_raster        the int8 raster: 100 occupied, 0 carved and not occupied, -1 neither
// Two bit planes (carved, occupied) cover every used frame's window: cell (x, y) is bit (x - x0) & 31 of word
// (y - y0) * wpr + ((x - x0) >> 5).  Integer work throughout; the results are unions of sets, so they do not depend
// on the order of frames, rows or threads.  scripts/map_ref.py restates ray_walk line for line.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "global_map.h"
#include "occupancy.h"

namespace icpmi {

constexpr int kRayMaxR = 4096;            // ICPMI_RAYCAST_MAX_R
constexpr int kRayLdsMaxR = 559;          // ICPMI_RAYCAST_LDS_MAX_R: the largest window within kRayLdsBytes
constexpr int kRayLdsBytes = 160 * 1024;  // all of a CU's LDS: one workgroup may take it (dynamic, past 64 KiB by attribute)
constexpr int kRayThreads = 1024;         // k_ray_carve_lds's workgroup

// A window row starts at the plane word that holds its first column, so its words are the plane's words: the bits
// of 2R + 3 cells behind a shift of at most 31.
constexpr int ray_window_row_words(int R) { return (2 * R + 3 + 62) / 32; }
constexpr int ray_window_words(int R) { return (2 * R + 3) * ray_window_row_words(R); }
static_assert(4 * ray_window_words(kRayLdsMaxR) <= kRayLdsBytes && 4 * ray_window_words(kRayLdsMaxR + 1) > kRayLdsBytes,
              "kRayLdsMaxR is the largest R whose window fits");

struct RayFrame {
    int64_t row0;     // the frame's first row in the store
    int32_t rows;
    int32_t sx, sy;   // its sensor cell: floor(t / resolution) in fp64, formed on the host
    int32_t pad;
};
static_assert(sizeof(RayFrame) == 24, "the frame table is uploaded as it is");

struct RayPlane {
    int32_t x0, y0;   // the cell of bit 0 of word 0
    int32_t w, h;     // cells
    int32_t wpr;      // words per row
};

struct RayBounds {    // in plane coordinates (cell - (x0, y0)); max < 0: no cell at all
    int32_t min_x, min_y, max_x, max_y;
    unsigned long long n_occupied, n_free;
};

// The walk from (x0, y0) to (x1, y1), in that direction: carve(x, y) for every cell of the line but the last.
template <class Carve>
__device__ __forceinline__ void ray_walk(int x0, int y0, int x1, int y1, Carve carve)
{
    const int dx = abs(x1 - x0), dy = abs(y1 - y0);
    const int sx = x1 > x0 ? 1 : (x1 < x0 ? -1 : 0), sy = y1 > y0 ? 1 : (y1 < y0 ? -1 : 0);
    int err = dx - dy, x = x0, y = y0;
    while (x != x1 || y != y1) {
        carve(x, y);
        const int e2 = 2 * err;
        if (e2 > -dy) err -= dy, x += sx;
        if (e2 < dx) err += dx, y += sy;
    }
}

// LDS: the plain atomic (testing the bit first measured slower).  Global: the word is tested first; most
// of it has been set by a neighbouring ray or frame already, and an atomic leaves L2.
__device__ __forceinline__ void ray_set_lds(unsigned *w, unsigned bit)
{
    __hip_atomic_fetch_or(w, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void ray_set_global(unsigned *w, unsigned bits)
{
    if ((__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bits) != bits)
        __hip_atomic_fetch_or(w, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A row's hit cell relative to its frame's sensor cell; false where the row casts no ray (kGridNone).  A hit lies
// within max_range of the sensor, so within R + 1 cells on each axis; the test keeps every walk inside the frame's
// window, and with it inside the plane, whatever the keys hold.
__device__ __forceinline__ bool ray_hit(unsigned long long key, const RayFrame &f, int R, int &ddx, int &ddy)
{
    if (key == kGridNone) return false;
    const long long ex = (long long)(int)((unsigned)(key >> 32) ^ 0x80000000u) - f.sx;
    const long long ey = (long long)(int)((unsigned)key ^ 0x80000000u) - f.sy;
    if (ex < -(R + 1) || ex > R + 1 || ey < -(R + 1) || ey > R + 1) return false;
    ddx = (int)ex;
    ddy = (int)ey;
    return true;
}

// keys: k_map_world's, indexed by store row.  Dynamic LDS: ray_window_words(R) words.
__global__ __launch_bounds__(kRayThreads) void k_ray_carve_lds(const unsigned long long *__restrict__ keys,
                                                               const RayFrame *__restrict__ frames, int R, RayPlane pl,
                                                               unsigned *__restrict__ carved, unsigned *__restrict__ occupied)
{
    extern __shared__ unsigned ray_window[];
    const RayFrame f = frames[blockIdx.x];
    if (f.rows == 0) return;
    const int side = 2 * R + 3, wwpr = ray_window_row_words(R), words = side * wwpr;
    const int wx0 = f.sx - (R + 1) - pl.x0, wy0 = f.sy - (R + 1) - pl.y0; // the window's corner in the plane, >= 0
    const int word0 = wx0 >> 5, cx = (wx0 & 31) + R + 1, cy = R + 1;      // the sensor cell in the window
    for (int i = (int)threadIdx.x; i < words; i += kRayThreads) ray_window[i] = 0u;
    __syncthreads();
    for (int r = (int)threadIdx.x; r < f.rows; r += kRayThreads) {
        int ddx, ddy;
        if (!ray_hit(keys[f.row0 + r], f, R, ddx, ddy)) continue;
        const int hx = wx0 + R + 1 + ddx, hy = wy0 + R + 1 + ddy;
        ray_set_global(occupied + (size_t)hy * pl.wpr + (hx >> 5), 1u << (hx & 31));
        ray_walk(cx, cy, cx + ddx, cy + ddy, [&](int x, int y) { ray_set_lds(ray_window + y * wwpr + (x >> 5), 1u << (x & 31)); });
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < words; i += kRayThreads) {
        const unsigned v = ray_window[i];
        const int row = i / wwpr, j = i - row * wwpr;
        if (v != 0u && word0 + j < pl.wpr) ray_set_global(carved + (size_t)(wy0 + row) * pl.wpr + word0 + j, v);
    }
}

__global__ __launch_bounds__(256) void k_ray_carve_global(const unsigned long long *__restrict__ keys,
                                                          const MapTile *__restrict__ tiles,
                                                          const RayFrame *__restrict__ frames, int R, RayPlane pl,
                                                          unsigned *__restrict__ carved, unsigned *__restrict__ occupied)
{
    const MapTile t = tiles[blockIdx.x];
    const RayFrame f = frames[t.frame];
    const int cx = f.sx - pl.x0, cy = f.sy - pl.y0; // the sensor cell in the plane, >= R + 1
    for (int r = (int)threadIdx.x; r < t.rows; r += 256) {
        int ddx, ddy;
        if (!ray_hit(keys[t.row0 + r], f, R, ddx, ddy)) continue;
        const int hx = cx + ddx, hy = cy + ddy;
        ray_set_global(occupied + (size_t)hy * pl.wpr + (hx >> 5), 1u << (hx & 31));
        ray_walk(cx, cy, hx, hy, [&](int x, int y) { ray_set_global(carved + (size_t)y * pl.wpr + (x >> 5), 1u << (x & 31)); });
    }
}

// out: {INT_MAX, INT_MAX, -1, -1, 0, 0} before the launch
__global__ __launch_bounds__(256) void k_ray_bounds(const unsigned *__restrict__ carved, const unsigned *__restrict__ occupied,
                                                    RayPlane pl, RayBounds *__restrict__ out)
{
    const size_t words = (size_t)pl.wpr * (size_t)pl.h;
    int min_x = INT32_MAX, min_y = INT32_MAX, max_x = -1, max_y = -1;
    unsigned long long n_occ = 0, n_free = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) {
        const unsigned o = occupied[i], c = carved[i] & ~o, any = o | c;
        if (any == 0u) continue;
        const int y = (int)(i / (size_t)pl.wpr), x = 32 * (int)(i - (size_t)y * (size_t)pl.wpr);
        min_x = min(min_x, x + __ffs((int)any) - 1);
        max_x = max(max_x, x + 31 - __clz((int)any));
        min_y = min(min_y, y);
        max_y = max(max_y, y);
        n_occ += (unsigned)__popc(o);
        n_free += (unsigned)__popc(c);
    }
    for (int d = 32; d > 0; d >>= 1) {
        min_x = min(min_x, __shfl_down(min_x, d));
        min_y = min(min_y, __shfl_down(min_y, d));
        max_x = max(max_x, __shfl_down(max_x, d));
        max_y = max(max_y, __shfl_down(max_y, d));
        n_occ += __shfl_down(n_occ, d);
        n_free += __shfl_down(n_free, d);
    }
    __shared__ int part[4][4];
    __shared__ unsigned long long part_n[4][2];
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = min_x, part[wave][1] = min_y, part[wave][2] = max_x, part[wave][3] = max_y;
        part_n[wave][0] = n_occ, part_n[wave][1] = n_free;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) {
        min_x = min(min_x, part[w][0]), min_y = min(min_y, part[w][1]);
        max_x = max(max_x, part[w][2]), max_y = max(max_y, part[w][3]);
        n_occ += part_n[w][0], n_free += part_n[w][1];
    }
    if (max_x < 0) return; // nothing marked in this workgroup's words
    atomicMin(&out->min_x, min_x);
    atomicMin(&out->min_y, min_y);
    atomicMax(&out->max_x, max_x);
    atomicMax(&out->max_y, max_y);
    atomicAdd(&out->n_occupied, n_occ);
    atomicAdd(&out->n_free, n_free);
}

// raster cell (i, j) is plane cell (bx + i, by + j); the raster's margin may reach past the plane
__global__ __launch_bounds__(256) void k_ray_raster(const unsigned *__restrict__ carved, const unsigned *__restrict__ occupied,
                                                    RayPlane pl, int bx, int by, int width, int height, int8_t *__restrict__ data)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)width * (size_t)height) return;
    const int j = (int)(idx / (size_t)width), i = (int)(idx - (size_t)j * (size_t)width);
    const int x = bx + i, y = by + j;
    int8_t v = -1;
    if (x >= 0 && x < pl.w && y >= 0 && y < pl.h) {
        const size_t w = (size_t)y * pl.wpr + (x >> 5);
        const unsigned bit = 1u << (x & 31);
        if (occupied[w] & bit) v = 100;
        else if (carved[w] & bit) v = 0;
    }
    data[idx] = v;
}

} // namespace icpmi
