// Host check of LoopPlan::cull_full (csrc/loop_plan.h): the culled full passes of the all-pairs engine against the condition
// written out flat -- sizes as literals, so that a changed constant in the header shows -- on the edges of the window of
// target sizes (12 and 13 splits, 3,072 and 3,073), of the source's row limits (sorted from 4,096; 2^25), and for every switch, rule and engine the
// condition reads; then what the field implies of the others, and that it moves no other field of the plan.
#include <cstdio>
#include <cstring>

#include "loop_plan.h"

using namespace icpmi;

namespace {

long failures = 0;
void fail(const LoopFacts &f, const char *what)
{
    if (++failures <= 20)
        printf("FAIL %s: n=%d splits=%d engine=%d culled=%d comm=%d rule=%d small=%d bounded=%d reuse=%d margin=%d lean=%d fuse_finish=%d "
               "cull_full=%d\n",
               what, f.n, f.nn_splits, f.nn_engine, (int)f.nn_pruned, (int)f.comm, (int)f.rule, (int)f.sw_small, (int)f.sw_bounded,
               (int)f.sw_reuse, (int)f.sw_margin, (int)f.sw_lean, (int)f.sw_fuse_finish, (int)f.sw_cull_full);
}

// list reuse as the loop derives it (tests/cpp/loop_plan_check.cpp holds the plan's field to the same chain)
bool ref_reuse(const LoopFacts &f)
{
    const bool mfma = f.nn_engine == ICPMI_SEARCH_MFMA_BF16, gate = f.rule != kRuleNone;
    const bool fused = mfma && !gate;
    const bool small = !f.comm && f.n > 0 && f.n <= 32768 && f.sw_small && mfma && !f.nn_pruned && f.nn_splits <= f.sw_small_max_splits;
    const bool pruned = fused && f.nn_pruned && f.n > 0;
    const bool bounded = fused && !small && f.n > 0 && (pruned || f.sw_bounded);
    return bounded && !pruned && f.sw_reuse;
}
// the rows in Morton order (sorted_rows_loop): outside the small-cloud kernel's sizes, from 4,096 rows, more than 12 splits
bool ref_sorted(const LoopFacts &f)
{
    const bool mfma = f.nn_engine == ICPMI_SEARCH_MFMA_BF16, gate = f.rule != kRuleNone;
    const bool small_sizes = !f.comm && f.n <= 32768 && f.nn_splits <= f.sw_small_max_splits;
    return mfma && !gate && !(f.nn_pruned && f.n > 0) && !small_sizes && f.n >= 4096 && f.nn_splits > 12;
}
bool ref_cull_full(const LoopFacts &f)
{
    return ref_reuse(f) && ref_sorted(f) && !f.comm && f.rule == kRuleNone && f.nn_splits > 12 && f.nn_splits <= 3072 && f.n < 33554432 &&
           f.sw_cull_full;
}

bool same_but_cull_full(const LoopPlan &a, const LoopPlan &b)
{
    return a.rule == b.rule && a.sharded == b.sharded && a.fused == b.fused && a.small == b.small && a.pruned == b.pruned &&
           a.sorted_rows_loop == b.sorted_rows_loop && a.sort_source == b.sort_source && a.bounded == b.bounded && a.reuse == b.reuse &&
           a.margin == b.margin && a.lean_on == b.lean_on && a.lean_from == b.lean_from && a.fused_tail == b.fused_tail &&
           a.resolve_waves == b.resolve_waves && a.rblocks == b.rblocks && a.sum_tree == b.sum_tree && a.rblocks2 == b.rblocks2 &&
           a.fin_blocks == b.fin_blocks && ((!a.error && !b.error) || (a.error && b.error && !strcmp(a.error, b.error)));
}

} // namespace

int main()
{
    static_assert(kKnnCullFromSplits == 12 && kCullMaxSplits == 3072 && kCullMaxRows == 33554432, "the window's limits");
    const int ns[] = {0, 1, 63, 64, 4095, 4096, 5000, 32768, 32769, 33000, 66000, 100000, 33554431, 33554432};
    const int splits[] = {1, 8, 9, 10, 12, 13, 14, 49, 3071, 3072, 3073, 4000};
    struct Engine { int engine; bool culled; } const engines[] = {
        {ICPMI_SEARCH_EXACT_F64, false}, {ICPMI_SEARCH_MFMA_BF16, false}, {ICPMI_SEARCH_MFMA_BF16, true}};
    const LoopRule rules[] = {kRuleNone, kRuleGate, kRuleRobust};
    long plans = 0, on = 0;
    for (const int n : ns)
        for (const int sp : splits)
            for (const Engine &e : engines)
                for (int comm = 0; comm < 2; ++comm)
                    for (const LoopRule rule : rules)
                        for (int sw = 0; sw < 128; ++sw) {
                            LoopFacts f;
                            f.n = n;
                            f.m = sp * 2048 - 5; // (2,048 targets to a split)
                            f.nn_engine = e.engine;
                            f.nn_pruned = e.culled;
                            f.nn_splits = sp;
                            f.comm = comm != 0;
                            f.rule = rule;
                            f.sw_small = sw & 1;
                            f.sw_bounded = sw & 2;
                            f.sw_reuse = sw & 4;
                            f.sw_margin = sw & 8;
                            f.sw_lean = sw & 16;
                            f.sw_fuse_finish = sw & 32;
                            f.sw_cull_full = sw & 64;
                            const LoopPlan p = make_loop_plan(f);
                            ++plans;
                            on += p.cull_full ? 1 : 0;
                            if (p.cull_full != ref_cull_full(f)) fail(f, "cull_full");
                            if (p.reuse != ref_reuse(f)) fail(f, "reuse");
                            if (p.sorted_rows_loop != ref_sorted(f)) fail(f, "sorted_rows_loop");
                            // what the field implies: the all-pairs engine's reuse loop on one GPU without a rule, never the culled
                            // engine's own loop nor the small-cloud kernel's
                            if (p.cull_full && !(p.reuse && p.sorted_rows_loop && p.bounded && p.fused && !p.pruned && !p.small && !p.sharded && p.rule == kRuleNone))
                                fail(f, "cull_full => reuse, sorted rows, bounded, fused, all pairs, general kernels, one GPU, no rule");
                            // the switch moves this field alone
                            LoopFacts g = f;
                            g.sw_cull_full = !f.sw_cull_full;
                            const LoopPlan q = make_loop_plan(g);
                            if (!same_but_cull_full(p, q)) fail(f, "the switch moved another field");
                            if (!f.sw_cull_full && p.cull_full) fail(f, "on with the switch off");
                        }
    // the window's edges by name, everything else at its default: 100,000 rows against 12 / 13 / 3,072 / 3,073 splits
    {
        LoopFacts f;
        f.n = 100000, f.nn_engine = ICPMI_SEARCH_MFMA_BF16;
        const struct { int splits; bool want; } edges[] = {{12, false}, {13, true}, {3072, true}, {3073, false}};
        for (const auto &e : edges) {
            f.nn_splits = e.splits, f.m = e.splits * 2048;
            if (make_loop_plan(f).cull_full != e.want) fail(f, "edge of the window");
        }
        f.nn_splits = 49, f.m = 100000;
        if (!make_loop_plan(f).cull_full) fail(f, "the headline's shape");
        f.n = kCullMaxRows;
        if (make_loop_plan(f).cull_full) fail(f, "the row limit");
        f.n = kCullMaxRows - 1;
        if (!make_loop_plan(f).cull_full) fail(f, "one below the row limit");
        // rows in the caller's order (fewer than 4,096; or ICPMI_SMALL=0 at the small-cloud kernel's sizes): all pairs
        f.n = 4095;
        if (make_loop_plan(f).cull_full) fail(f, "unsorted rows");
        f.n = 4096;
        if (!make_loop_plan(f).cull_full) fail(f, "the first sorted size");
        f.n = 20000, f.nn_splits = 14, f.m = 14 * 2048, f.sw_small = false, f.sw_small_max_splits = 16;
        if (make_loop_plan(f).cull_full) fail(f, "general kernels at the small-cloud kernel's sizes");
    }
    if (!on) ++failures, printf("FAIL no plan had culled full passes\n");
    // a default-constructed plan and default facts: off and on
    if (LoopPlan{}.cull_full || !LoopFacts{}.sw_cull_full) ++failures, printf("FAIL defaults\n");
    if (failures) {
        printf("%ld failures\n", failures);
        return 1;
    }
    printf("ok %ld plans, %ld with culled full passes\n", plans, on);
    return 0;
}
