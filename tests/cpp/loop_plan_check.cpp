// Host check of csrc/loop_plan.h: make_loop_plan and the per-pass decisions against the chain of conditions they
// replaced, written out flat below in the order the registration loop derived them (sizes as literals, so that a changed
// constant in the header shows), over the edges of every size the decisions look at and every combination of switches;
// then the implications between the plan's fields, and the lean passes' bookkeeping pass by pass.
#include <cstdio>
#include <cstring>
#include <vector>

#include "loop_plan.h"

using namespace icpmi;

namespace {

struct Ref {
    bool sharded, fused, small, pruned, sorted_rows_loop, bounded, reuse, margin, lean_on, sum_tree;
    int lean_from, rblocks, rblocks2, fin_blocks, resolve_waves;
    const char *error;
};

int ref_resolve_waves(int n) { return n <= 32768 ? 8 : 0; }
int ref_resolve_blocks(int n)
{
    const int w = ref_resolve_waves(n);
    const int per = w > 0 ? 4 * w : 4 * 16;
    return (n + per - 1) / per;
}
int ref_reduce_blocks(int cu_count, int n) { return std::max(1, std::min(cu_count, (n + 255) / 256)); }

// the loop's derivation before the plan: `gate` / `kind` are the rule, the sw_* what the environment readers returned
Ref reference(const LoopFacts &f)
{
    Ref r{};
    const int n = f.n;
    const bool gate = f.rule != kRuleNone, kind = f.rule == kRuleRobust;
    const bool mfma = f.nn_engine == ICPMI_SEARCH_MFMA_BF16;
    const bool small_target = f.sw_small && mfma && !f.nn_pruned && f.nn_splits <= f.sw_small_max_splits;
    const bool sharded_run = f.comm;
    const bool fused = mfma && !gate;
    const bool small = !sharded_run && n > 0 && n <= 32768 && small_target;
    const int rblocks = small ? (n + 32 - 1) / 32 : (fused ? ref_resolve_blocks(n) : ref_reduce_blocks(f.cu_count, n));
    const bool sum_tree = rblocks >= 1024;
    const int rblocks2 = sum_tree ? (rblocks + 16 - 1) / 16 : 0;
    if (gate && kind && sum_tree && !small) r.error = "internal: a robust pass of %d partial rows";
    const int fin_blocks = sum_tree ? rblocks2 : rblocks;
    const bool sharded = f.comm;
    const bool pruned = fused && f.nn_pruned && n > 0;
    const bool small_regime = !sharded_run && n <= 32768 && f.nn_splits <= f.sw_small_max_splits;
    const bool sorted_rows_loop = fused && !pruned && !small && !small_regime && n >= 4096 && f.nn_splits > 12;
    const bool bounded_loop = fused && !small && n > 0 && (pruned || f.sw_bounded);
    if (!r.error && pruned && !bounded_loop) r.error = "internal: the culled engine needs the bounded resolve kernels";
    const bool reuse = bounded_loop && !pruned && f.sw_reuse;
    const bool margin = reuse && !gate && ref_resolve_waves(n) == 0 && f.sw_margin;
    const bool lean_on = reuse && !sharded_run && !gate && f.sw_fuse_finish && sum_tree && f.sw_lean;
    const int lean_from = lean_on ? f.sw_lean_from : 0;
    r.sharded = sharded, r.fused = fused, r.small = small, r.pruned = pruned, r.sorted_rows_loop = sorted_rows_loop;
    r.bounded = bounded_loop, r.reuse = reuse, r.margin = margin, r.lean_on = lean_on, r.sum_tree = sum_tree;
    r.lean_from = lean_from, r.rblocks = rblocks, r.rblocks2 = rblocks2, r.fin_blocks = fin_blocks;
    r.resolve_waves = ref_resolve_waves(n);
    return r;
}
bool ref_fuse_step(const LoopFacts &f, int final_pass) { return f.comm && f.n > 0 && !final_pass; }
bool ref_fuse_finish(const LoopFacts &f, int final_pass)
{
    return !f.comm && f.n > 0 && !final_pass && !(f.rule != kRuleNone) && f.sw_fuse_finish;
}

long failures = 0;
void expect(bool ok, const LoopFacts &f, const char *what)
{
    if (ok) return;
    if (++failures <= 20)
        printf("FAIL %s: n=%d splits=%d engine=%d culled=%d comm=%d rule=%d profile=%d small=%d/%d bounded=%d reuse=%d margin=%d "
               "lean=%d from=%d fuse_finish=%d\n",
               what, f.n, f.nn_splits, f.nn_engine, (int)f.nn_pruned, (int)f.comm, (int)f.rule, f.profile, (int)f.sw_small,
               f.sw_small_max_splits, (int)f.sw_bounded, (int)f.sw_reuse, (int)f.sw_margin, (int)f.sw_lean, f.sw_lean_from,
               (int)f.sw_fuse_finish);
}
bool same_text(const char *a, const char *b) { return (!a && !b) || (a && b && !strcmp(a, b)); }

void check_plan(const LoopFacts &f)
{
    const Ref r = reference(f);
    const LoopPlan p = make_loop_plan(f);
    expect(p.sharded == r.sharded, f, "sharded");
    expect(p.fused == r.fused, f, "fused");
    expect(p.small == r.small, f, "small");
    expect(p.pruned == r.pruned, f, "pruned");
    expect(p.sorted_rows_loop == r.sorted_rows_loop, f, "sorted_rows_loop");
    expect(p.sort_source == (r.pruned || r.sorted_rows_loop), f, "sort_source");
    expect(p.bounded == r.bounded, f, "bounded");
    expect(p.reuse == r.reuse, f, "reuse");
    expect(p.margin == r.margin, f, "margin");
    expect(p.lean_on == r.lean_on, f, "lean_on");
    expect(p.lean_from == r.lean_from, f, "lean_from");
    expect(p.sum_tree == r.sum_tree, f, "sum_tree");
    expect(p.rblocks == r.rblocks, f, "rblocks");
    expect(p.rblocks2 == r.rblocks2, f, "rblocks2");
    expect(p.fin_blocks == r.fin_blocks, f, "fin_blocks");
    expect(p.resolve_waves == r.resolve_waves, f, "resolve_waves");
    expect(p.rule == f.rule, f, "rule");
    expect(same_text(p.error, r.error), f, "error");
    for (int final_pass = 0; final_pass < 2; ++final_pass) {
        expect(fuse_step(p, f.n, final_pass) == ref_fuse_step(f, final_pass), f, "fuse_step");
        expect(fuse_finish(p, f.n, final_pass) == ref_fuse_finish(f, final_pass), f, "fuse_finish");
    }
    // what the fields imply of each other
    expect(!p.margin || p.reuse, f, "margin => reuse");
    expect(!p.reuse || p.bounded, f, "reuse => bounded");
    expect(!p.bounded || p.fused, f, "bounded => fused");
    expect(!p.pruned || p.bounded || p.error, f, "pruned => bounded or the error");
    expect(!p.lean_on || (p.reuse && p.sum_tree && p.rule == kRuleNone && !p.sharded), f, "lean_on => reuse, sum_tree, no rule, one GPU");
    expect(!p.small || (!p.bounded && !p.sort_source), f, "small => neither bounded nor sorted");
    const bool robust_refused = p.error && !strcmp(p.error, "internal: a robust pass of %d partial rows");
    expect(robust_refused == (f.rule == kRuleRobust && r.sum_tree && !r.small), f, "the robust refusal's place");
}

// the loop's bookkeeping of lean passes before lean_next, for one pass P (from 1)
bool ref_lean_next(int P, int final_pass, int lean_from, const std::vector<unsigned> &want_known)
{
    bool lean_nxt = false;
    if (!final_pass) {
        if (lean_from) lean_nxt = P + 1 >= lean_from;
        else if (P >= 6 && (int)want_known.size() >= P - 2) lean_nxt = lean_pass(P + 1, want_known[P - 4], want_known[P - 3]);
    }
    return lean_nxt;
}

void check_lean()
{
    const int passes = 12;
    const unsigned seqs[][passes] = {
        {900, 40, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0},   // settles early: lean from the first pass the rule allows
        {900, 40, 3, 1, 0, 0, 0, 2, 0, 0, 0, 0},   // a row wants a list again in between
        {900, 800, 700, 600, 500, 400, 300, 200, 100, 50, 20, 10}, // never settles
        {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},      // (the first passes list every row whatever the words say)
        {5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
    };
    const int lags[] = {2, 3, 4, 12}; // counts known when pass P is queued: P - 2 (the queue loop), one or two fewer (late), none
    const int froms[] = {0, 2, 5};
    int lean_seen = 0;
    for (const auto &seq : seqs)
        for (const int lag : lags)
            for (const int from : froms) {
                std::vector<unsigned> known;
                for (int P = 1; P <= passes; ++P) {
                    while ((int)known.size() < P - lag) known.push_back(seq[known.size()]);
                    const int final_pass = P == passes;
                    const bool want = ref_lean_next(P, final_pass, from, known);
                    const bool got = lean_next(P, final_pass, from, known.data(), (int)known.size());
                    lean_seen += got ? 1 : 0;
                    if (want != got) {
                        ++failures;
                        printf("FAIL lean_next: pass %d lag %d from %d: %d, reference %d\n", P, lag, from, (int)got, (int)want);
                    }
                }
            }
    if (!lean_seen) ++failures, printf("FAIL lean_next: no sequence had a lean pass\n");
    // with the queue loop's lag and no hook the schedule is lean_schedule's (list_reuse.h)
    for (const auto &seq : seqs) {
        bool sched[passes];
        lean_schedule(seq, passes, sched);
        std::vector<unsigned> known;
        for (int P = 1; P < passes - 1; ++P) {
            while ((int)known.size() < P - 2) known.push_back(seq[known.size()]);
            if (lean_next(P, 0, 0, known.data(), (int)known.size()) != sched[P]) ++failures, printf("FAIL lean_schedule: pass %d\n", P + 1);
        }
    }
}

} // namespace

int main()
{
    const int ns[] = {0, 1, 31, 32, 4095, 4096, 32736, 32737, 32768, 32769, 65536, 100000, 1048575, 1048576};
    const int splits[] = {1, 7, 8, 9, 12, 13, 49};
    struct Engine { int engine; bool culled; } const engines[] = {
        {ICPMI_SEARCH_EXACT_F64, false}, {ICPMI_SEARCH_MFMA_BF16, false}, {ICPMI_SEARCH_MFMA_BF16, true}};
    const LoopRule rules[] = {kRuleNone, kRuleGate, kRuleRobust};
    const int lean_froms[] = {0, 2, 5};
    long plans = 0;
    for (const int n : ns)
        for (const int sp : splits)
            for (const Engine &e : engines)
                for (int comm = 0; comm < 2; ++comm)
                    for (const LoopRule rule : rules)
                        for (int profile = 0; profile <= 2; profile += 2)
                            for (int sw = 0; sw < 64; ++sw)
                                for (const int from : lean_froms) {
                                    LoopFacts f;
                                    f.n = n;
                                    f.m = sp * 2048 - 5; // (2,048 targets to a split)
                                    f.nn_engine = e.engine;
                                    f.nn_pruned = e.culled;
                                    f.nn_splits = (f.m + 2047) / 2048;
                                    f.cu_count = 256;
                                    f.comm = comm != 0;
                                    f.rule = rule;
                                    f.profile = profile;
                                    f.sw_small = sw & 1;
                                    f.sw_bounded = sw & 2;
                                    f.sw_reuse = sw & 4;
                                    f.sw_margin = sw & 8;
                                    f.sw_lean = sw & 16;
                                    f.sw_fuse_finish = sw & 32;
                                    f.sw_lean_from = from;
                                    check_plan(f);
                                    ++plans;
                                }
    // ICPMI_SMALL_MAX_SPLITS at its ends (the grid above ran its default)
    for (const int limit : {0, 16})
        for (const int n : ns)
            for (const int sp : splits) {
                LoopFacts f;
                f.n = n, f.m = sp * 2048 - 5, f.nn_splits = sp, f.nn_engine = ICPMI_SEARCH_MFMA_BF16, f.sw_small_max_splits = limit;
                check_plan(f);
                ++plans;
            }
    check_lean();
    if (failures) {
        printf("%ld failures\n", failures);
        return 1;
    }
    printf("ok %ld plans\n", plans);
    return 0;
}
