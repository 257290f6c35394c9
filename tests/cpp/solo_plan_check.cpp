// Host check of solo passes as the plan and the queue loop see them (csrc/loop_plan.h: LoopPlan::solo_on, solo_next): the
// field against its condition written out flat -- sizes as literals, so that a changed constant in the header shows -- on
// both edges of every term; that its switch and its hook move no other field; solo_next against a slow restatement over
// random count sequences; that a solo tail implies a lean pass behind it by lean_next's own rule; and the test hook.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "loop_plan.h"

using namespace icpmi;

namespace {

long failures = 0;
void fail(const LoopFacts &f, const char *what)
{
    if (++failures <= 20)
        printf("FAIL %s: n=%d splits=%d engine=%d culled=%d comm=%d rule=%d profile=%d small=%d bounded=%d reuse=%d margin=%d lean=%d "
               "fuse_finish=%d solo=%d solo_from=%d\n",
               what, f.n, f.nn_splits, f.nn_engine, (int)f.nn_pruned, (int)f.comm, (int)f.rule, f.profile, (int)f.sw_small, (int)f.sw_bounded,
               (int)f.sw_reuse, (int)f.sw_margin, (int)f.sw_lean, (int)f.sw_fuse_finish, (int)f.sw_solo, f.sw_solo_from);
}

// the chain of conditions, flat (tests/cpp/loop_plan_check.cpp holds the fields before solo_on to the same chain)
bool ref_solo_on(const LoopFacts &f)
{
    const bool mfma = f.nn_engine == ICPMI_SEARCH_MFMA_BF16, gate = f.rule != kRuleNone;
    const bool fused = mfma && !gate;
    const bool small = !f.comm && f.n > 0 && f.n <= 32768 && f.sw_small && mfma && !f.nn_pruned && f.nn_splits <= f.sw_small_max_splits;
    const bool pruned = fused && f.nn_pruned && f.n > 0;
    const bool bounded = fused && !small && f.n > 0 && (pruned || f.sw_bounded);
    const bool reuse = bounded && !pruned && f.sw_reuse;
    const bool margin = reuse && !gate && f.n > 32768 && f.sw_margin;
    const bool fused_tail = !f.comm && !gate && f.sw_fuse_finish;
    const int rblocks = (f.n + 63) / 64; // (a fused general pass of more than 32,768 rows: a partial row per 64)
    const bool sum_tree = rblocks >= 1024;
    const bool lean_on = reuse && fused_tail && sum_tree && f.sw_lean;
    // one group row per workgroup of 1,024 rows, one row per thread of at most 128 workgroups
    return lean_on && margin && f.n >= 65473 && f.n <= 131072 && f.profile < 2 && f.sw_solo;
}

bool same_but_solo(const LoopPlan &a, const LoopPlan &b)
{
    return a.rule == b.rule && a.sharded == b.sharded && a.fused == b.fused && a.small == b.small && a.pruned == b.pruned &&
           a.sorted_rows_loop == b.sorted_rows_loop && a.sort_source == b.sort_source && a.bounded == b.bounded && a.reuse == b.reuse &&
           a.margin == b.margin && a.lean_on == b.lean_on && a.lean_from == b.lean_from && a.fused_tail == b.fused_tail &&
           a.resolve_waves == b.resolve_waves && a.rblocks == b.rblocks && a.sum_tree == b.sum_tree && a.rblocks2 == b.rblocks2 &&
           a.fin_blocks == b.fin_blocks && a.cull_full == b.cull_full && ((!a.error && !b.error) || (a.error && b.error && !strcmp(a.error, b.error)));
}

// solo_next, slowly: the tail of pass P is the solo kernel when the host has read the counts of passes P - 3 and P - 2 (it
// has read P - 2 counts when it queues pass P) and both passes found every row certified
bool slow_solo_next(int P, int final_pass, int from, const std::vector<unsigned> &uncert, int known)
{
    if (final_pass) return false;
    if (from) return P >= from;
    for (int q = P - 3; q <= P - 2; ++q) {
        if (q < 1 || q > known) return false;
        if (uncert[(size_t)q - 1] != 0u) return false;
    }
    return true;
}

} // namespace

int main()
{
    static_assert(kFinishThreads == 1024 && kFinishBlocksMax == 128 && kSumGroup == 16 && kSumTreeFrom == 1024 && kResolveWW * kResolveQ == 64,
                  "the sizes the window comes from");
    const int ns[] = {0, 64, 32768, 32769, 65472, 65473, 66000, 100000, 131071, 131072, 131073, 200000};
    const int splits[] = {8, 12, 13, 20, 49};
    struct Engine { int engine; bool culled; } const engines[] = {
        {ICPMI_SEARCH_EXACT_F64, false}, {ICPMI_SEARCH_MFMA_BF16, false}, {ICPMI_SEARCH_MFMA_BF16, true}};
    const LoopRule rules[] = {kRuleNone, kRuleGate, kRuleRobust};
    long plans = 0, on = 0;
    for (const int n : ns)
        for (const int sp : splits)
            for (const Engine &e : engines)
                for (int comm = 0; comm < 2; ++comm)
                    for (const LoopRule rule : rules)
                        for (int profile = 0; profile < 3; ++profile)
                            for (int sw = 0; sw < 128; ++sw) {
                                LoopFacts f;
                                f.n = n;
                                f.m = sp * 2048 - 5;
                                f.nn_engine = e.engine;
                                f.nn_pruned = e.culled;
                                f.nn_splits = sp;
                                f.comm = comm != 0;
                                f.rule = rule;
                                f.profile = profile;
                                f.sw_small = sw & 1;
                                f.sw_bounded = sw & 2;
                                f.sw_reuse = sw & 4;
                                f.sw_margin = sw & 8;
                                f.sw_lean = sw & 16;
                                f.sw_fuse_finish = sw & 32;
                                f.sw_solo = sw & 64;
                                const LoopPlan p = make_loop_plan(f);
                                if (p.error) continue; // (a refused form launches nothing)
                                ++plans;
                                on += p.solo_on ? 1 : 0;
                                if (p.solo_on != ref_solo_on(f)) fail(f, "solo_on");
                                if (p.solo_on && !(p.lean_on && p.margin && p.reuse && p.fused_tail && p.sum_tree && !p.pruned && !p.small &&
                                                   !p.sharded && p.rule == kRuleNone && p.fin_blocks == finish_transform_blocks(n) &&
                                                   p.fin_blocks == (n + 1023) / 1024 && p.rblocks == (n + 63) / 64))
                                    fail(f, "solo_on => lean passes, the match margin, one GPU, no rule, a group row per workgroup");
                                if (p.solo_from != 0) fail(f, "the hook, unset");
                                // the switch moves this field alone; the hook moves solo_from alone, and only where the plan is on
                                LoopFacts g = f;
                                g.sw_solo = !f.sw_solo;
                                if (!same_but_solo(p, make_loop_plan(g))) fail(f, "the switch moved another field");
                                if (!f.sw_solo && p.solo_on) fail(f, "on with the switch off");
                                g = f;
                                g.sw_solo_from = 3;
                                const LoopPlan h = make_loop_plan(g);
                                if (!same_but_solo(p, h) || h.solo_on != p.solo_on || h.solo_from != (p.solo_on ? 3 : 0)) fail(f, "the hook");
                            }
    // the edges by name, everything else at its default (the headline's engine, 20 splits)
    {
        LoopFacts f;
        f.nn_engine = ICPMI_SEARCH_MFMA_BF16, f.nn_splits = 20, f.m = 40000;
        const struct { int n; bool want; } edges[] = {{65472, false}, {65473, true}, {66000, true}, {100000, true}, {131072, true}, {131073, false}};
        for (const auto &e : edges) {
            f.n = e.n;
            if (make_loop_plan(f).solo_on != e.want) fail(f, "edge of the window");
        }
        f.n = 100000;
        f.profile = 1;
        if (!make_loop_plan(f).solo_on) fail(f, "profile level 1");
        f.profile = 2;
        if (make_loop_plan(f).solo_on) fail(f, "profile level 2");
        f.profile = 0;
        f.sw_margin = false;
        if (make_loop_plan(f).solo_on) fail(f, "without the match margin");
        f.sw_margin = true, f.sw_lean = false;
        if (make_loop_plan(f).solo_on) fail(f, "without lean passes");
        f.sw_lean = true, f.sw_fuse_finish = false;
        if (make_loop_plan(f).solo_on) fail(f, "without the fused tail");
        f.sw_fuse_finish = true, f.rule = kRuleGate;
        if (make_loop_plan(f).solo_on) fail(f, "under a gate");
        f.rule = kRuleNone, f.nn_pruned = true;
        if (make_loop_plan(f).solo_on) fail(f, "the culled engine");
        f.nn_pruned = false, f.comm = true;
        if (make_loop_plan(f).solo_on) fail(f, "sharded");
    }
    if (!on) ++failures, printf("FAIL no plan had solo passes\n");
    if (LoopPlan{}.solo_on || LoopPlan{}.solo_from || !LoopFacts{}.sw_solo || LoopFacts{}.sw_solo_from) ++failures, printf("FAIL defaults\n");

    // solo_next over random count sequences: mostly zeros with a few stragglers, counts known up to a random pass
    std::mt19937 rng(20261021u);
    long decisions = 0, solo = 0;
    for (int trial = 0; trial < 20000; ++trial) {
        const int passes = 1 + (int)(rng() % 40);
        std::vector<unsigned> uncert((size_t)passes), want((size_t)passes);
        const int settle = (int)(rng() % 12);
        for (int q = 0; q < passes; ++q) {
            uncert[(size_t)q] = q < 2 ? 66000u : (q < settle || rng() % 9 == 0) ? 1u + (unsigned)(rng() % 70000) : 0u;
            // the rows listed again are among the rows not certified
            want[(size_t)q] = q < 2 ? 66000u : uncert[(size_t)q] ? (unsigned)(rng() % (uncert[(size_t)q] + 1u)) : 0u;
        }
        const int from = rng() % 5 == 0 ? 2 + (int)(rng() % 8) : 0;
        for (int P = 1; P <= passes + 2; ++P) {
            const int known = std::min(passes, std::max(0, P - 2 - (int)(rng() % 2))); // (P - 2, or one fewer: a count not yet read)
            for (int final_pass = 0; final_pass < 2; ++final_pass) {
                const bool got = solo_next(P, final_pass, from, uncert.data(), known);
                ++decisions;
                solo += got ? 1 : 0;
                if (got != slow_solo_next(P, final_pass, from, uncert, known)) {
                    if (++failures <= 20) printf("FAIL solo_next: trial %d P=%d final=%d from=%d known=%d\n", trial, P, final_pass, from, known);
                }
                // by the counts, a solo tail is never before pass 6 and the pass behind it is lean by lean_next's own rule
                if (got && !from) {
                    if (P < 6) ++failures, printf("FAIL solo before pass 6: trial %d P=%d\n", trial, P);
                    if (!lean_next(P, 0, 0, want.data(), known)) ++failures, printf("FAIL solo without lean: trial %d P=%d\n", trial, P);
                }
                if (got && final_pass) ++failures, printf("FAIL the post-loop pass has no solo tail\n");
            }
        }
    }
    if (!solo) ++failures, printf("FAIL no solo decision\n");
    // the hook: every tail from the k-th pass on, whatever the counts say or however few are known
    {
        const unsigned none[1] = {66000u};
        for (int k = 2; k < 12; ++k)
            for (int P = 1; P < 40; ++P)
                if (solo_next(P, 0, k, none, 0) != (P >= k) || solo_next(P, 1, k, none, 0)) ++failures, printf("FAIL hook k=%d P=%d\n", k, P);
    }
    if (failures) {
        printf("%ld failures\n", failures);
        return 1;
    }
    printf("ok %ld plans, %ld with solo passes; %ld decisions, %ld solo\n", plans, on, decisions, solo);
    return 0;
}
