// Host check of the packed row list's index arithmetic (lidar_slam_from_scratch_amd/csrc/list_reuse.h): random masks of n
// rows, n not a multiple of 64, at densities 0, 1e-4, 1 %, 50 % and 1.  The list is formed the way k_row_list (kernels.h)
// forms it -- workgroups of `T` words, each counting the words below it with T strided partial counts, then every word
// expanded at its own prefix -- and must be exactly the ascending indices of the set bits, and the count their number.
// row_list_kth_bit is also checked on its own against a bit-by-bit walk.  Prints "ok <cases> <rows listed>" or the first
// difference; exit 1 then.
#include <cstdio>
#include <random>
#include <vector>

#include "list_reuse.h"

int main()
{
    constexpr int T = 256; // words per workgroup of k_row_list
    std::mt19937_64 rng(2718281828ull);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const double dens[] = {0.0, 1e-4, 0.01, 0.5, 1.0};
    const int sizes[] = {1, 63, 65, 1000, 40000 + 17, 100000 - 1, 100001, 16384 * 3 + 5, 1000003};
    long cases = 0, listed = 0;
    for (const int n : sizes) {
        for (const double p : dens) {
            const int nw = (n + 63) / 64;
            std::vector<unsigned long long> mask(nw, 0ull);
            std::vector<int> want;
            for (int i = 0; i < n; ++i)
                if (p >= 1.0 || (p > 0.0 && U(rng) < p)) {
                    mask[i >> 6] |= 1ull << (i & 63);
                    want.push_back(i);
                }
            // popcount and k-th set bit, word by word
            for (int g = 0; g < nw; ++g) {
                int c = 0;
                for (int b = 0; b < 64; ++b)
                    if (mask[g] >> b & 1ull) {
                        if (icpmi::row_list_kth_bit(mask[g], c) != b) {
                            std::printf("KTH n %d p %g word %d: bit %d of %016llx -> %d, not %d\n", n, p, g, c, mask[g], icpmi::row_list_kth_bit(mask[g], c), b);
                            return 1;
                        }
                        ++c;
                    }
                if (icpmi::row_list_popcount(mask[g]) != c) {
                    std::printf("POPCOUNT n %d p %g word %d\n", n, p, g);
                    return 1;
                }
            }
            // the list, the kernel's way
            std::vector<int> rows(n + 1, -1);
            int count = -1;
            for (int g0 = 0; g0 < nw; g0 += T) {
                int below = 0, above = 0, own = 0;
                for (int tid = 0; tid < T; ++tid) {
                    below += icpmi::row_list_count(mask.data(), tid, g0, T);
                    above += icpmi::row_list_count(mask.data(), g0 + T + tid, nw, T);
                }
                int at = below;
                for (int tid = 0; tid < T && g0 + tid < nw; ++tid) at += icpmi::row_list_expand(mask[g0 + tid], g0 + tid, rows.data(), at);
                own = at - below;
                const int total = below + own + above;
                if (count >= 0 && total != count) {
                    std::printf("COUNT n %d p %g: workgroup at word %d has %d, an earlier one %d\n", n, p, g0, total, count);
                    return 1;
                }
                count = total;
            }
            if (count != (int)want.size() || count != icpmi::row_list_count(mask.data(), 0, nw, 1)) {
                std::printf("COUNT n %d p %g: %d, not %zu\n", n, p, count, want.size());
                return 1;
            }
            for (int k = 0; k < count; ++k)
                if (rows[k] != want[k]) {
                    std::printf("ROW n %d p %g: rows[%d] = %d, not %d\n", n, p, k, rows[k], want[k]);
                    return 1;
                }
            if (rows[count] != -1) {
                std::printf("OVERRUN n %d p %g: rows[%d] written\n", n, p, count);
                return 1;
            }
            if (p >= 1.0 && count != n) { // (k_row_list's flag for "every row is listed" is count == n)
                std::printf("FULL n %d: count %d\n", n, count);
                return 1;
            }
            ++cases;
            listed += count;
        }
    }
    std::printf("ok %ld %ld\n", cases, listed);
    return 0;
}
