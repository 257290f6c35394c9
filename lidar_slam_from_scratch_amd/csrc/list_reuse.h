// list_reuse.h -- the arithmetic of list reuse in the bounded ICP passes (RowBounds, kernels.h), for host and device: the
// kernels that move the rows use it, and tests/cpp/list_reuse_check.cpp checks it against an fp64 brute force.
#pragma once
#if defined(__HIPCC__)
#define ICPMI_HD __host__ __device__
#else
#define ICPMI_HD
#endif

namespace icpmi {

// The radius a row's list is built for: sqrt(ub) and twice the skin, the skin being the larger of `frac` x sqrt(ub) and
// twice the row's displacement by the step just taken, at most sqrt(ub).  (1 + 1e-12: see list_certified.)
ICPMI_HD inline double list_radius(const double sq, const double disp, const double frac)
{
    double skin = frac * sq > 2.0 * disp ? frac * sq : 2.0 * disp;
    skin = skin < sq ? skin : sq;
    return (sq + 2.0 * skin) * (1.0 + 1e-12);
}

// A list built at x_b for radius r_b holds every target within r_b of x_b.  The row now sits at y, d = |y - x_b|, and its
// nearest neighbour is within sqrt(ub) of y (ub: the exact distance to its previous match), hence within sqrt(ub) + d of
// x_b.  sq = sqrt(ub) and d are fp64 sums and roots of a few correctly rounded terms, each within 1e-15 of its exact
// value: the factor 1 + 1e-12 on the left covers them.  NaN r_b (a list not to be kept) fails the comparison.
ICPMI_HD inline bool list_certified(const double sq, const double d, const double r_b) { return (sq + d) * (1.0 + 1e-12) <= r_b; }

} // namespace icpmi
