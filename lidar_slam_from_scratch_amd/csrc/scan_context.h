// scan_context.h -- Scan Context place-recognition descriptor and its shifted cosine
// distance on the GPU (reference core/scan_context.hpp).
//
//   k_scan_context      scan_context.hpp:44-82   20 rings x 60 sectors, max height per bin
//   k_sc_distances      scan_context.hpp:90-142  one query against a history of descriptors,
//                                                min over the 60 column shifts of 1 - cosine
//   k_sc_distances_shift                         the same distance and the smallest shift that attains it (the yaw
//                                                between the two scans to half a sector; not in the reference, which
//                                                drops the argmin at :94-99)
//
// The max per bin is order independent, so an LDS 64-bit atomic max on an order-preserving
// integer image of the double gives the reference's result bit for bit (up to atan2's last
// ulp at a sector boundary).  The distance sums run in the reference's (ring, sector) order
// with unfused multiply-adds, one thread per (descriptor, shift).  Both bodies are device functions
// (sc_describe, sc_distance) that the loop-closure store's kernels (loop_store.h) run as well.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace icpmi {

constexpr int kScRings = 20, kScSectors = 60, kScCells = kScRings * kScSectors;

__device__ __forceinline__ unsigned long long sc_encode(double v) // order-preserving
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double sc_decode(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// The body of k_scan_context, shared with k_loop_describe (loop_store.h): the descriptor of rows
// cloud[0 .. n) into desc, by the 1024 threads of one workgroup.  (The LDS is declared here, not passed in: so the
// kernels' code is what it was before the body moved.)
__device__ __forceinline__ void sc_describe(const double *__restrict__ cloud, int n, double *__restrict__ desc)
{
    __shared__ unsigned long long bins[kScCells];
    const double kMaxRange = 80.0;                         // scan_context.hpp:29
    const double ring_size = kMaxRange / kScRings;         // :47
    const double sector_size = 2.0 * 3.14159265358979323846 / kScSectors; // :48
    const unsigned long long empty = sc_encode(-1.7976931348623157e308); // :45
    for (int e = threadIdx.x; e < kScCells; e += 1024) bins[e] = empty;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 1024) {
        const double x = cloud[3 * i], y = cloud[3 * i + 1], z = cloud[3 * i + 2];
        const double range = __dsqrt_rn(x * x + y * y);              // :56
        const double angle = atan2(y, x) + 3.14159265358979323846;   // :57
        if (range > kMaxRange || range < 0.1) continue;              // :59
        int ring = (int)(range / ring_size);                         // :62
        int sector = (int)(angle / sector_size);                     // :63
        ring = ring < 0 ? 0 : (ring > kScRings - 1 ? kScRings - 1 : ring);
        sector = sector < 0 ? 0 : (sector > kScSectors - 1 ? kScSectors - 1 : sector);
        if (z == z) atomicMax(&bins[ring * kScSectors + sector], sc_encode(z)); // :69-71 (NaN never wins)
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kScCells; e += 1024) {
        const double v = sc_decode(bins[e]);
        desc[e] = v < -1000.0 ? 0.0 : v;                              // :75-81
    }
}

__global__ __launch_bounds__(1024) void k_scan_context(const double *__restrict__ cloud, int n,
                                                       double *__restrict__ desc)
{
    sc_describe(cloud, n, desc);
}

// The body of k_sc_distances, shared with k_loop_candidates (loop_store.h): column_shifted_distance of
// descriptor `other` to `query` by the 64 threads of one workgroup (thread `shift` evaluates one shift).  Every
// lane returns the min over the shifts.
__device__ __forceinline__ double sc_distance(const double *__restrict__ query, const double *__restrict__ other)
{
    __shared__ double a[kScCells], b[kScCells];
    for (int e = threadIdx.x; e < kScCells; e += 64) {
        a[e] = query[e];
        b[e] = other[e];
    }
    __syncthreads();
    const int shift = threadIdx.x;
    double dist = 1.7976931348623157e308; // scan_context.hpp:91
    if (shift < kScSectors) {
        double sum_ab = 0.0, sum_aa = 0.0, sum_bb = 0.0; // :122-124
        for (int i = 0; i < kScRings; ++i)
            for (int j = 0; j < kScSectors; ++j) {
                int js = j + shift;
                js = js >= kScSectors ? js - kScSectors : js;
                const double va = a[i * kScSectors + j], vb = b[i * kScSectors + js];
                sum_ab += va * vb;
                sum_aa += va * va;
                sum_bb += vb * vb;
            }
        const double norm = __dsqrt_rn(sum_aa) * __dsqrt_rn(sum_bb); // :137
        dist = norm < 1e-10 ? 1.0 : 1.0 - sum_ab / norm;            // :138-141
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(dist, off, 64);
        dist = o < dist ? o : dist;
    }
    return dist;
}

// grid = history size, 64 threads
__global__ __launch_bounds__(64) void k_sc_distances(const double *__restrict__ query,
                                                     const double *__restrict__ hist, int count,
                                                     double *__restrict__ out)
{
    const int d = blockIdx.x;
    if (d >= count) return;
    const double dist = sc_distance(query, hist + (size_t)d * kScCells);
    if (threadIdx.x == 0) out[d] = dist;
}

// sc_distance that keeps the argmin: every lane returns the same min over the shifts, bit for bit, and in `shift` the
// SMALLEST shift that attains it (scan_context.hpp:94-99 runs upward with a strict <).  The per-lane sums restate
// sc_distance's, in its order, and are not shared with it: k_sc_distances and k_loop_candidates keep their code.  The
// reduction is sc_distance's butterfly with the shift riding along, one more 32-bit exchange per step; the distance's
// own update is unchanged, so with a NaN among the per-shift distances the value is still what sc_distance returns
// (the shift is then some lane's, 0..59).  Lanes 60-63 enter as the reference's loop starts, (DBL_MAX, no shift
// chosen: 0): no shift's distance equals DBL_MAX, so they never win a tie against one.
__device__ __forceinline__ double sc_distance_shift(const double *__restrict__ query, const double *__restrict__ other,
                                                    int &shift_out)
{
    __shared__ double a[kScCells], b[kScCells];
    for (int e = threadIdx.x; e < kScCells; e += 64) {
        a[e] = query[e];
        b[e] = other[e];
    }
    __syncthreads();
    const int lane = threadIdx.x;
    double dist = 1.7976931348623157e308; // scan_context.hpp:91
    int shift = 0;
    if (lane < kScSectors) {
        shift = lane;
        double sum_ab = 0.0, sum_aa = 0.0, sum_bb = 0.0; // :122-124
        for (int i = 0; i < kScRings; ++i)
            for (int j = 0; j < kScSectors; ++j) {
                int js = j + lane;
                js = js >= kScSectors ? js - kScSectors : js;
                const double va = a[i * kScSectors + j], vb = b[i * kScSectors + js];
                sum_ab += va * vb;
                sum_aa += va * va;
                sum_bb += vb * vb;
            }
        const double norm = __dsqrt_rn(sum_aa) * __dsqrt_rn(sum_bb); // :137
        dist = norm < 1e-10 ? 1.0 : 1.0 - sum_ab / norm;            // :138-141
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(dist, off, 64);
        const int os = __shfl_xor(shift, off, 64);
        shift = (o < dist || (o == dist && os < shift)) ? os : shift;
        dist = o < dist ? o : dist;
    }
    shift_out = shift;
    return dist;
}

// grid = history size, 64 threads
__global__ __launch_bounds__(64) void k_sc_distances_shift(const double *__restrict__ query,
                                                           const double *__restrict__ hist, int count,
                                                           double *__restrict__ out, int32_t *__restrict__ shift_out)
{
    const int d = blockIdx.x;
    if (d >= count) return;
    int shift;
    const double dist = sc_distance_shift(query, hist + (size_t)d * kScCells, shift);
    if (threadIdx.x == 0) {
        out[d] = dist;
        shift_out[d] = shift;
    }
}

} // namespace icpmi
