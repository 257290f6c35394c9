// Prints the plan of a registration call (csrc/loop_plan.h: make_loop_plan) for facts given on the command line, so that a
// test can choose its source sizes from the plan instead of from literals.
//
//   loop_plan_print engine=mfma pruned=0 splits=15 cu=256 rule=none small=1 n=1:140000
//
// engine: exact | mfma; rule: none | gate | robust; small: the ICPMI_SMALL switch; n=A:B: every source size from A to B.
// One line per run of consecutive sizes with the same plan:
//   n_first n_last rblocks sum_tree rblocks2 fin_blocks small fused pruned resolve_waves
// and, first, one line "constants kMfmaMinQueries kSmallMaxQueries kSumGroup kSumTreeFrom".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "loop_plan.h"

using namespace icpmi;

int main(int argc, char **argv)
{
    LoopFacts f;
    f.nn_engine = ICPMI_SEARCH_MFMA_BF16;
    long n0 = 1, n1 = 1;
    for (int a = 1; a < argc; ++a) {
        const char *eq = strchr(argv[a], '=');
        if (!eq) { fprintf(stderr, "expected key=value, got %s\n", argv[a]); return 2; }
        const size_t kl = (size_t)(eq - argv[a]);
        const char *v = eq + 1;
        auto key = [&](const char *k) { return strlen(k) == kl && !strncmp(argv[a], k, kl); };
        if (key("engine")) {
            if (!strcmp(v, "exact")) f.nn_engine = ICPMI_SEARCH_EXACT_F64;
            else if (!strcmp(v, "mfma")) f.nn_engine = ICPMI_SEARCH_MFMA_BF16;
            else { fprintf(stderr, "engine=exact|mfma\n"); return 2; }
        } else if (key("pruned")) f.nn_pruned = atoi(v) != 0;
        else if (key("splits")) f.nn_splits = atoi(v);
        else if (key("cu")) f.cu_count = atoi(v);
        else if (key("comm")) f.comm = atoi(v) != 0;
        else if (key("small")) f.sw_small = atoi(v) != 0;
        else if (key("small_max_splits")) f.sw_small_max_splits = atoi(v);
        else if (key("rule")) {
            if (!strcmp(v, "none")) f.rule = kRuleNone;
            else if (!strcmp(v, "gate")) f.rule = kRuleGate;
            else if (!strcmp(v, "robust")) f.rule = kRuleRobust;
            else { fprintf(stderr, "rule=none|gate|robust\n"); return 2; }
        } else if (key("n")) {
            char *end = nullptr;
            n0 = n1 = strtol(v, &end, 10);
            if (*end == ':') n1 = strtol(end + 1, nullptr, 10);
        } else { fprintf(stderr, "unknown fact %s\n", argv[a]); return 2; }
    }
    if (n0 < 1 || n1 < n0 || n1 > 100000000) { fprintf(stderr, "n=A or n=A:B with 1 <= A <= B <= 1e8\n"); return 2; }
    printf("constants %d %d %d %d\n", kMfmaMinQueries, kSmallMaxQueries, kSumGroup, kSumTreeFrom);
    LoopPlan run{};
    long first = 0;
    auto same = [](const LoopPlan &a, const LoopPlan &b) {
        return a.rblocks == b.rblocks && a.sum_tree == b.sum_tree && a.rblocks2 == b.rblocks2 && a.fin_blocks == b.fin_blocks &&
               a.small == b.small && a.fused == b.fused && a.pruned == b.pruned && a.resolve_waves == b.resolve_waves &&
               (a.error != nullptr) == (b.error != nullptr);
    };
    auto print = [&](long last) {
        printf("%ld %ld %d %d %d %d %d %d %d %d%s\n", first, last, run.rblocks, (int)run.sum_tree, run.rblocks2, run.fin_blocks,
               (int)run.small, (int)run.fused, (int)run.pruned, run.resolve_waves, run.error ? " refused" : "");
    };
    for (long n = n0; n <= n1; ++n) {
        f.n = (int)n;
        const LoopPlan p = make_loop_plan(f);
        if (n == n0) { run = p; first = n; continue; }
        if (!same(p, run)) {
            print(n - 1);
            run = p;
            first = n;
        }
    }
    print(n1);
    return 0;
}
