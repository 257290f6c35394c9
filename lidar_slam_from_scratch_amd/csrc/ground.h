// ground.h -- ground segmentation of a scan in its sensor frame (the reference names it as future work,
// README.md:304, and has no code for it).  A polar grid of n_rings x n_sectors bins over [min_range, max_range]:
//     pass 1   zmin[bin] = the least z of the bin's rows
//     walk     per sector, outward over the rings: a bin's zmin is taken as the ground there if it lies within
//              step_tol + max_slope * (distance to the last accepted ring) of the ground so far; every bin gets a ground
//              height, its own, the last accepted ring's, or the prior -sensor_height
//     pass 2   a row's height over its bin's ground: GROUND, OBSTACLE (within the clearance band) or IGNORED
// One workgroup of 1024 threads per scan, the bins in LDS as 64-bit words in sc_describe's pattern (scan_context.h):
// the minimum is an LDS atomic min on sc_encode's order-preserving image of the double, so it does not depend on the
// row order.  fp64, unfused, in the order written: scripts/ground_ref.py restates it byte for byte (atan2's last ulp
// at a sector boundary aside).  Bandwidth: 24 B read twice per row (the second time from L2), 1 B written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occupancy.h"
#include "scan_context.h"

namespace icpmi {

constexpr int kGroundThreads = 1024;
constexpr int kGroundLdsBytes = 160 * 1024; // all of a CU's LDS (dynamic, past 64 KiB by attribute)
constexpr int kGroundMaxBins = 20400;       // ICPMI_GROUND_MAX_BINS: e.g. 80 x 255; 640 B stay for the kernel's static LDS
static_assert(8 * kGroundMaxBins + 640 <= kGroundLdsBytes, "the bins of the largest grid fit one CU's LDS");

constexpr uint8_t kGroundObstacle = 0, kGroundGround = 1, kGroundIgnored = 2; // ICPMI_GROUND_*
constexpr unsigned long long kGroundEmpty = ~0ull; // no finite z encodes to it (sc_encode of a NaN's bits)

struct GroundParams {
    int32_t n_rings, n_sectors;
    double min_range, max_range, sensor_height, max_slope, step_tol, height_tol, clear_min, clear_max;
};

struct GroundFrame {
    int64_t row0; // the scan's first row in `store`
    int32_t rows;
    int32_t pad;
};
static_assert(sizeof(GroundFrame) == 16, "the frame table is uploaded as it is");

struct GroundCounts { // per scan; a scan holds fewer than 2^31 rows
    unsigned n_ground, n_obstacle, n_ignored, bins_accepted;
};

// The bin of a row, -1 where it enters none.  A quotient at or past the count (or a NaN from a ring_size that
// underflowed) takes the last ring or sector: the clamp, made before the cast so that the cast is always defined.
__device__ __forceinline__ int ground_bin(double x, double y, double z, const GroundParams &p, double ring_size,
                                          double sector_size)
{
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return -1;
    const double range = __dsqrt_rn(x * x + y * y);
    const double angle = atan2(y, x) + 3.14159265358979323846;
    if (range < p.min_range || range > p.max_range) return -1;
    const double qr = (range - p.min_range) / ring_size, qs = angle / sector_size;
    int ring = qr < (double)p.n_rings ? (int)qr : p.n_rings - 1;
    int sector = qs < (double)p.n_sectors ? (int)qs : p.n_sectors - 1;
    ring = ring < 0 ? 0 : ring;
    sector = sector < 0 ? 0 : sector;
    return ring * p.n_sectors + sector;
}

// grid = scans, kGroundThreads threads, dynamic LDS of 8 * n_rings * n_sectors bytes.  labels (and height, if not
// null) are indexed by store row; ground_z (if not null) holds n_rings * n_sectors doubles per scan, ring-major.
__global__ __launch_bounds__(kGroundThreads) void k_ground_label(const double *__restrict__ store,
                                                                 const GroundFrame *__restrict__ frames, GroundParams p,
                                                                 uint8_t *__restrict__ labels, double *__restrict__ height,
                                                                 double *__restrict__ ground_z, GroundCounts *__restrict__ counts)
{
    extern __shared__ unsigned long long ground_bins[];
    __shared__ unsigned tally[4];
    const GroundFrame f = frames[blockIdx.x];
    const int bins = p.n_rings * p.n_sectors;
    const double ring_size = (p.max_range - p.min_range) / (double)p.n_rings;
    const double sector_size = 2.0 * 3.14159265358979323846 / (double)p.n_sectors;
    const double *in = store + 3 * (size_t)f.row0;
    if (threadIdx.x < 4) tally[threadIdx.x] = 0u;
    for (int e = (int)threadIdx.x; e < bins; e += kGroundThreads) ground_bins[e] = kGroundEmpty;
    __syncthreads();
    for (int i = (int)threadIdx.x; i < f.rows; i += kGroundThreads) {
        const double x = in[3 * (size_t)i], y = in[3 * (size_t)i + 1], z = in[3 * (size_t)i + 2];
        const int b = ground_bin(x, y, z, p, ring_size, sector_size);
        if (b >= 0) atomicMin(&ground_bins[b], sc_encode(z));
    }
    __syncthreads();
    for (int s = (int)threadIdx.x; s < p.n_sectors; s += kGroundThreads) {
        double gz = -p.sensor_height, gr = 0.0;
        unsigned accepted = 0u;
        for (int r = 0; r < p.n_rings; ++r) {
            const int e = r * p.n_sectors + s;
            const unsigned long long w = ground_bins[e];
            if (w != kGroundEmpty) {
                const double zmin = sc_decode(w);
                const double rc = p.min_range + ((double)r + 0.5) * ring_size;
                const double lim = p.step_tol + p.max_slope * (rc - gr);
                if (fabs(zmin - gz) <= lim) gz = zmin, gr = rc, ++accepted;
            }
            ground_bins[e] = (unsigned long long)__double_as_longlong(gz); // the bin's ground height over its minimum
            if (ground_z) ground_z[(size_t)blockIdx.x * (size_t)bins + (size_t)e] = gz;
        }
        if (accepted) atomicAdd(&tally[3], accepted);
    }
    __syncthreads();
    unsigned n_ground = 0u, n_obstacle = 0u, n_ignored = 0u;
    for (int i = (int)threadIdx.x; i < f.rows; i += kGroundThreads) {
        const double x = in[3 * (size_t)i], y = in[3 * (size_t)i + 1], z = in[3 * (size_t)i + 2];
        const int b = ground_bin(x, y, z, p, ring_size, sector_size);
        uint8_t label = kGroundIgnored;
        double h = __longlong_as_double(0x7ff8000000000000ll); // a row that entered no bin
        if (b >= 0) {
            h = z - __longlong_as_double((long long)ground_bins[b]);
            if (h <= p.height_tol) label = kGroundGround;
            else if (p.clear_min <= h && h <= p.clear_max) label = kGroundObstacle;
        }
        labels[(size_t)f.row0 + (size_t)i] = label;
        if (height) height[(size_t)f.row0 + (size_t)i] = h;
        n_ground += label == kGroundGround, n_obstacle += label == kGroundObstacle, n_ignored += label == kGroundIgnored;
    }
    for (int d = 32; d > 0; d >>= 1) {
        n_ground += __shfl_down(n_ground, d);
        n_obstacle += __shfl_down(n_obstacle, d);
        n_ignored += __shfl_down(n_ignored, d);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&tally[0], n_ground);
        atomicAdd(&tally[1], n_obstacle);
        atomicAdd(&tally[2], n_ignored);
    }
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = GroundCounts{tally[0], tally[1], tally[2], tally[3]};
}

// keys: k_map_world's for `n` consecutive store rows, formed with an open height band; labels: those rows' labels.
// A row that is not OBSTACLE marks nothing and casts no ray.
__global__ __launch_bounds__(256) void k_ground_mask(unsigned long long *__restrict__ keys, const uint8_t *__restrict__ labels,
                                                     size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && labels[i] != kGroundObstacle) keys[i] = kGridNone;
}

} // namespace icpmi
