// Host check of list reuse's arithmetic (lidar_slam_from_scratch_amd/csrc/list_reuse.h) against an fp64 brute force:
// random targets, rows whose list is built at x_b for list_radius(...) -- the list modelled as every target within R_b of
// x_b, the least the coarse pass guarantees -- then moved by a random drift (many of them right at the certificate's
// edge).  Whenever list_certified keeps the list, the row's exact nearest neighbour (smallest fp64 distance, ties to the
// lowest index, the resolve's rule) must be in it.  Prints "ok <kept> <rebuilt>" or the first counterexample; exit 1 then.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "list_reuse.h"

static double sqd(const double *a, const double *b)
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}

int main(int argc, char **argv)
{
    const int trials = argc > 1 ? atoi(argv[1]) : 20000;
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    long kept = 0, rebuilt = 0;
    for (int t = 0; t < trials; ++t) {
        const double scale = std::pow(10.0, (int)(rng() % 7) - 3); // 1e-3 .. 1e3
        const double off = (rng() % 3 == 0) ? 1e4 * scale : 0.0;  // far from the origin: large coordinates, small distances
        const int m = 16 + (int)(rng() % 400);
        std::vector<double> tg(3 * m);
        for (int j = 0; j < m; ++j)
            for (int a = 0; a < 3; ++a) tg[3 * j + a] = off + scale * U(rng);
        if (rng() % 4 == 0) // duplicated targets: exact ties
            for (int j = 1; j < m; j += 3)
                for (int a = 0; a < 3; ++a) tg[3 * j + a] = tg[3 * (j - 1) + a];
        double xb[3], y[3];
        for (int a = 0; a < 3; ++a) xb[a] = off + scale * U(rng);
        // the list's build: bound from some target (the previous match), skin from a random displacement and fraction
        const int jp = (int)(rng() % m);
        const double sq0 = std::sqrt(sqd(xb, &tg[3 * jp]));
        const double frac = (rng() % 5) * 0.25, disp = scale * 0.1 * std::fabs(U(rng)) * (rng() % 2);
        const double rb = icpmi::list_radius(sq0, disp, frac);
        // the move: a random direction, length drawn up to and across the radius the certificate allows
        double dir[3], nd = 0.0;
        for (int a = 0; a < 3; ++a) dir[a] = U(rng), nd += dir[a] * dir[a];
        nd = std::sqrt(nd);
        const double len = rb * std::fabs(U(rng)) * (rng() % 2 ? 1.0 : 0.5);
        for (int a = 0; a < 3; ++a) y[a] = xb[a] + dir[a] / nd * len;
        // the previous match now: the target nearest to x_b (what the pass that built the list resolved), or any other
        int jm = 0;
        for (int j = 1; j < m; ++j)
            if (sqd(xb, &tg[3 * j]) < sqd(xb, &tg[3 * jm])) jm = j;
        if (rng() % 3 == 0) jm = (int)(rng() % m);
        const double ub = sqd(y, &tg[3 * jm]);
        const double dx = y[0] - xb[0], dy = y[1] - xb[1], dz = y[2] - xb[2];
        const double d = std::sqrt((dx * dx + dy * dy) + dz * dz);
        if (!icpmi::list_certified(std::sqrt(ub), d, rb)) {
            ++rebuilt;
            continue;
        }
        ++kept;
        int best = 0;
        for (int j = 1; j < m; ++j)
            if (sqd(y, &tg[3 * j]) < sqd(y, &tg[3 * best])) best = j; // (strict: ties keep the lowest index)
        // in the list: exact distance to x_b within R_b, checked in long double
        long double e = 0.0L;
        for (int a = 0; a < 3; ++a) {
            const long double q = (long double)tg[3 * best + a] - (long double)xb[a];
            e += q * q;
        }
        if (std::sqrt(e) > (long double)rb) {
            std::printf("MISS trial %d: nearest %d at %.17Lg from x_b, R_b %.17g (ub %.17g, d %.17g)\n", t, best, std::sqrt(e), rb, ub, d);
            return 1;
        }
    }
    std::printf("ok %ld %ld\n", kept, rebuilt);
    return kept > trials / 10 && rebuilt > trials / 10 ? 0 : 1;
}
