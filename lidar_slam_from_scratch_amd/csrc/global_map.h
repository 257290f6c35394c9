// global_map.h -- the node's map from its kept scans and optimised poses (slam_viz/src/ros/slam_node.cpp):
//     downsampled_clouds_.push_back(curr)                                    :71, :123
//     rebuild_recent_clouds: world points of the last 20 frames              :187-194
//     build_final_global_map: every frame moved by its final pose            :196-209
//     rebuild_occupancy_grid: cleared, then one insert per frame with that   :223-229
//         frame's own translation as the sensor position
// The kept scans live in one contiguous N x 3 fp64 arena (icpmi_map, capi.hip), frame after frame.  A host-built
// tile table cuts every frame into tiles of at most kMapTileRows rows; k_map_world runs one workgroup per tile of
// whatever frames a call asks for, so one launch moves them all.  A tile's pose is uniform across its workgroup
// (scalar loads); per row the kernel writes the world point (Rigid34::apply, the ICP loop's formula) and, for the
// cell set, the row's key (grid_cell_key, k_grid_keys's predicate).  An HBM stream: 24 B read, 24 B written
// when world points are wanted, 8 B per key.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.h"
#include "occupancy.h"

namespace icpmi {

constexpr int kMapTileRows = 1024; // 4 rows per thread of a 256-thread workgroup

struct MapTile {
    int64_t row0;  // the tile's first row in the store
    int32_t frame; // the frame it belongs to
    int32_t rows;  // 1 .. kMapTileRows
};
static_assert(sizeof(MapTile) == 16, "the tile table is uploaded as it is");

// tiles: the launch's tiles (one workgroup each); poses: 16 doubles (row-major 4 x 4) per frame from frame0 on;
// output row of store row r: r - out_row0.  world (N x 3) and keys (N) may each be null.  g.sx, g.sy are unused:
// the sensor is the tile's frame's translation (slam_node.cpp:227).
__global__ __launch_bounds__(256) void k_map_world(const double *__restrict__ store, const MapTile *__restrict__ tiles,
                                                   const double *__restrict__ poses, int32_t frame0, int64_t out_row0,
                                                   double *__restrict__ world, unsigned long long *__restrict__ keys,
                                                   GridParams g)
{
    constexpr int B = kMapTileRows / 256;
    const MapTile t = tiles[blockIdx.x];
    const Rigid34 P = Rigid34::load(poses + 16 * (size_t)(t.frame - frame0));
    const double *in = store + 3 * (size_t)t.row0;
    const size_t o0 = (size_t)(t.row0 - out_row0);
    double x[B], y[B], z[B];
#pragma unroll
    for (int b = 0; b < B; ++b) { // every load of the thread first
        const int r = (int)threadIdx.x + 256 * b;
        x[b] = y[b] = z[b] = 0.0;
        if (r < t.rows) x[b] = in[3 * r], y[b] = in[3 * r + 1], z[b] = in[3 * r + 2];
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const int r = (int)threadIdx.x + 256 * b;
        if (r >= t.rows) break;
        double px, py, pz;
        P.apply(x[b], y[b], z[b], px, py, pz);
        const size_t o = o0 + (size_t)r;
        if (world) {
            world[3 * o] = px;
            world[3 * o + 1] = py;
            world[3 * o + 2] = pz;
        }
        if (keys) keys[o] = grid_cell_key(px, py, pz, g, P.t0, P.t1);
    }
}

} // namespace icpmi
