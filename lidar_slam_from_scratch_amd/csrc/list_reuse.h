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

// ---- the match margin (RowBounds::scan, kernels.h; k_nn_resolve_bounded<true>, nn_bounded.h) ---------------------------
// When the exact resolve scans a row at x_s it sees the exact distance of every target in the row's listed slots, and
// the list holds every target within `cover` of x_s.  With d2 the distance of the nearest scanned target OTHER than the
// winner, every target but the winner is at least g = min(d2, cover) away from x_s.  At a later pass the row sits at y,
// delta = |y - x_s|, and its kept match is at sqrt(ub) exactly: every other target is at least g - delta away, so while
// sqrt(ub) + delta < g the kept match is the unique nearest target at y and the exact resolve, which starts from it at
// bd = ub, would return it unchanged -- no scan, no list, no coarse pass for that row.

// The radius around the row's place y within which a list built at x_b for r_b holds every target: r_b - |y - x_b|
// (d = |y - x_b|, 0 for a list built where the row is).  The factors push both terms the safe way by more than their
// roundings (1e-15 relative, see list_certified).  NaN r_b (a call's first pass) gives NaN.
ICPMI_HD inline double list_cover(const double r_b, const double d) { return r_b * (1.0 - 1e-12) - d * (1.0 + 1e-12); }

// g from the SQUARED distance of the nearest scanned target other than the winner (`none`: no other target was scanned)
// and the list's cover; the root is pulled down by more than its rounding.  NaN cover gives NaN, which never certifies.
ICPMI_HD inline double match_margin(const double d2sq, const bool none, const double cover)
{
    if (!(cover == cover)) return cover;
    const double d2 = __builtin_sqrt(d2sq) * (1.0 - 1e-12);
    return (none || cover < d2) ? cover : d2;
}

// sq = sqrt(ub), delta = |y - x_s|: fp64 roots of sums of a few correctly rounded terms, each within 1e-15 of its exact
// value, like g's ingredients; 1 + 1e-12 covers them.  Strict: a tie (a duplicated target point: d2 == the match's own
// distance) never certifies.  NaN in g, sq or delta fails the comparison; so does sq = +Inf (a row without a match).
ICPMI_HD inline bool match_certified(const double sq, const double delta, const double g) { return (sq + delta) * (1.0 + 1e-12) < g; }

// ---- the packed list of the rows listed again (RowBounds::mask, k_row_list in kernels.h) -------------------------------
// The kernel that moves the rows leaves one 64-bit word per group of 64 consecutive rows, bit b of word g set where row
// 64 g + b is listed again.  The packed list is the set bits' rows in ascending order: row_list_count gives a word's place
// in it, row_list_expand writes a word's rows there.  tests/cpp/row_list_check.cpp runs the three on the host.
ICPMI_HD inline int row_list_popcount(unsigned long long w)
{
    w = w - ((w >> 1) & 0x5555555555555555ull);
    w = (w & 0x3333333333333333ull) + ((w >> 2) & 0x3333333333333333ull);
    w = (w + (w >> 4)) & 0x0f0f0f0f0f0f0f0full;
    return (int)((w * 0x0101010101010101ull) >> 56);
}

// set bits of words[lo], words[lo + step], ... below `hi` (the device: one thread's share of a prefix; the host: step 1)
ICPMI_HD inline int row_list_count(const unsigned long long *words, const int lo, const int hi, const int step)
{
    int c = 0;
    for (int g = lo; g < hi; g += step) c += row_list_popcount(words[g]);
    return c;
}

// position of the k-th set bit of w, k = 0 for the lowest (k < popcount(w)): by halves, on the counts below each half
ICPMI_HD inline int row_list_kth_bit(unsigned long long w, int k)
{
    int pos = 0;
    for (int width = 32; width > 0; width >>= 1) {
        const unsigned long long low = w & ((1ull << width) - 1ull);
        const int c = row_list_popcount(low);
        if (k >= c) {
            k -= c;
            w >>= width;
            pos += width;
        } else {
            w = low;
        }
    }
    return pos;
}

// rows[at ...] = the rows of group `g` whose bit is set in `w`, ascending; returns how many
ICPMI_HD inline int row_list_expand(const unsigned long long w, const int g, int *rows, const int at)
{
    const int c = row_list_popcount(w);
    for (int k = 0; k < c; ++k) rows[at + k] = 64 * g + row_list_kth_bit(w, k);
    return c;
}

// ---- lean passes (the loop of icpmi_align in capi.hip; k_sum_groups in kernels.h) ------------------------
// want(p): the rows whose bit the mover of pass p - 1 left set in RowBounds::mask, the rows pass p lists.  A LEAN pass
// launches neither k_row_list nor the coarse kernel: a row that wanted a list then has cnt == 0 and takes the resolve's
// exhaustive search, exact with ties (nn_bounded.h, `over`) -- slower for that row, never another bit.  The host decides
// pass p when it queues the tail of pass p - 1; it has then seen the progress word of pass p - 3, so want(p - 4) and
// want(p - 3), published by kernels that completed, are the two latest counts it knows.  Pass p is lean when both are 0
// and neither is a call's first or second pass (those list every row whatever the words say).  Passes are numbered from 1.
ICPMI_HD inline bool lean_pass(const int pass, const unsigned want_older, const unsigned want_newer)
{
    return pass - 4 >= 3 && want_older == 0u && want_newer == 0u;
}

// lean[p - 1] for the passes p = 1 ... passes of a call whose counts are want[p - 1] = want(p): the rule applied the way
// the host loop applies it, each pass decided from the two counts known by then.  Returns the number of lean passes.
ICPMI_HD inline int lean_schedule(const unsigned *want, const int passes, bool *lean)
{
    int c = 0;
    for (int p = 1; p <= passes; ++p) {
        lean[p - 1] = p >= 5 && lean_pass(p, want[p - 5], want[p - 4]);
        c += lean[p - 1] ? 1 : 0;
    }
    return c;
}

} // namespace icpmi
