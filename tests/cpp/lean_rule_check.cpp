// Host check of the lean-pass rule (csrc/list_reuse.h: lean_pass, lean_schedule), built with the host compiler by
// tests/test_lean_rule_math.py.  Each case is a call's counts want(1 ... N) -- the rows each pass wanted listed -- and the
// passes that must be lean, written down by hand from the rule: pass p is lean when want(p - 4) and want(p - 3) are both 0
// and p - 4 >= 3.  Prints "ok <cases>" or the first difference; exit 1 then.
#include <cstdio>
#include <vector>

#include "list_reuse.h"

struct Case {
    const char *name;
    std::vector<unsigned> want;
    std::vector<int> lean; // the lean passes, from 1
};

int main()
{
    const unsigned n = 66000u;
    const std::vector<Case> cases = {
        {"never zero", {n, n, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5}, {}},
        {"zero from pass 3", {n, n, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {7, 8, 9, 10, 11, 12}},
        {"zero, zero, then non-zero", {n, n, 5, 0, 0, 7, 0, 0, 0, 0, 0, 0}, {8, 11, 12}},
        {"alternating", {n, n, 0, 3, 0, 3, 0, 3, 0, 3, 0, 3}, {}},
        {"zeros only in passes 1-2", {0, 0, 4, 4, 4, 4, 4, 4, 4, 4}, {}},
        {"zeros in passes 1-4 only", {0, 0, 0, 0, 4, 4, 4, 4, 4, 4}, {7}},
        {"one pass", {0}, {}},
        {"two passes", {0, 0}, {}},
        {"three passes", {0, 0, 0}, {}},
        {"six passes, all zero", {0, 0, 0, 0, 0, 0}, {}},
        {"seven passes, all zero", {0, 0, 0, 0, 0, 0, 0}, {7}},
    };
    for (const Case &c : cases) {
        const int N = (int)c.want.size();
        // (guards around the array: lean_schedule must read want[0 ... N - 1] only and write lean[0 ... N - 1] only)
        std::vector<unsigned> w(N + 2, 0xFFFFFFFFu);
        for (int p = 0; p < N; ++p) w[p + 1] = c.want[p];
        bool lean[64];
        for (bool &b : lean) b = true;
        const int count = icpmi::lean_schedule(w.data() + 1, N, lean + 1);
        std::vector<int> got;
        for (int p = 1; p <= N; ++p)
            if (lean[p]) got.push_back(p);
        if (got != c.lean || count != (int)c.lean.size() || !lean[0] || !lean[N + 1]) {
            std::printf("case '%s': lean passes", c.name);
            for (int p : got) std::printf(" %d", p);
            std::printf(" (count %d), expected", count);
            for (int p : c.lean) std::printf(" %d", p);
            std::printf("\n");
            return 1;
        }
    }
    // the rule itself at its edges: the older count must be of pass 3 or later, and any count above 0 makes the pass full
    if (icpmi::lean_pass(6, 0u, 0u) || !icpmi::lean_pass(7, 0u, 0u) || icpmi::lean_pass(7, 1u, 0u) || icpmi::lean_pass(7, 0u, 1u) ||
        icpmi::lean_pass(1000, 0u, 0x80000000u) || !icpmi::lean_pass(1000, 0u, 0u)) {
        std::printf("lean_pass: an edge of the rule is wrong\n");
        return 1;
    }
    std::printf("ok %d\n", (int)cases.size());
    return 0;
}
