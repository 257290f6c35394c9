// loop_plan.h -- the form of one registration call as data (the loop of icpmi_align in capi.hip), for host and device
// compilers alike: no HIP in here, no getenv.  capi.hip fills a LoopFacts from the context, the prepared engine, the gate
// and the environment switches, make_loop_plan() derives everything the call's launches depend on, and
// tests/cpp/loop_plan_check.cpp holds the derivation to the flat chain of conditions it replaced.  The sizes the plan
// depends on are defined here, once; the kernels use the same names.
#pragma once
#include <algorithm>

#include "../../include/icp_mi355x.h"
#include "list_reuse.h"

namespace icpmi {

// ---- sizes the kernels and the plan share --------------------------------------------------------------------------
constexpr int kTile = 32;                         // queries / targets per MFMA tile
constexpr int kCoarseQT = 2;                      // 32-query tiles per wave
constexpr int kCoarseWaves = 8;                   // waves per workgroup
constexpr int kCoarseQueries = kTile * kCoarseQT * kCoarseWaves; // queries per workgroup
constexpr int kResolveWW = 4; // waves per workgroup = Q * WW queries per partial row of normal-equation terms
constexpr int kResolveQ = 16; // queries per wave of k_nn_resolve / k_nn_resolve_bounded (nn_mfma.h)
constexpr int kSmallQ = 32;   // rows (queries) per workgroup of the small-cloud kernel (icp_small.h)
// (k_sum_groups, kernels.h: from kSumTreeFrom partial rows on they are first added in groups of kSumGroup)
constexpr int kSumGroup = 16;
constexpr int kSumTreeFrom = 1024;
// the kernels that sum, step and move the rows in one launch (k_finish_step_transform*, kernels.h): threads per workgroup,
// and the most workgroups of a launch -- each repeats the final sum.  (Round 3: 128.  With the rows' bounds formed there
// too (RowBounds) the row part is worth spreading over more CUs than the repeated sums cost: 32 / 64 / 128 / 256
// workgroups 22.1 / 18.2 / 16.5 / 16.5 us at 100k rows.)
constexpr int kFinishThreads = 1024;
constexpr int kFinishBlocksMax = 128;
inline int finish_transform_blocks(int n)
{
    return std::max(1, std::min(kFinishBlocksMax, (n + kFinishThreads - 1) / kFinishThreads));
}

// (AUTO takes the exact fp64 kernels for sources of fewer rows: engine_for in capi.hip)
constexpr int kMfmaMinQueries = 64;

// The box test of nn_culled.h (32-row tile against 2,048-target split) on the all-pairs engine: the target's 20-NN pass and
// the two passes of a registration that list every row (LoopPlan::cull_full) run over the surviving pairs once the target
// has more than kKnnCullFromSplits splits -- the size from which AUTO takes the culled engine (kAutoCulledFrom, capi.hip) --
// and at most kCullMaxSplits: the splits whose running sums fit k_nn_coarse_groups' LDS beside its 36 KiB of staging
// (2 x 3072 + 1 words of the 64 KiB a workgroup may have: 6.3M targets; nn_culled.h holds the assertion).  That kernel
// keeps a list's length in 20 bits (tiles of 32 rows): sources of fewer than kCullMaxRows rows.
constexpr int kKnnCullFromSplits = 12;
constexpr int kCullMaxSplits = 3072;
constexpr int kCullMaxRows = 1 << 25;

// Small clouds (the reference's real callers: filtered scans of 5-20k points): search, residuals and
// pose update of the rows in ONE kernel per iteration (icp_small.h) when the target is at most
// kSmallMaxSplits splits and the source at most kSmallMaxQueries rows (beyond, the general path's 512-query
// units amortise the operand reads better).  ICPMI_SMALL=0 switches the path off (A/B runs, parity
// test).
constexpr int kSmallMaxQueries = 32768;
// The small-cloud kernel's workgroup takes 32 rows through ALL splits, so its time grows with rows x splits where the
// general path's grows with the units on the chip: measured (scripts/engine_threshold.py, profiles/r4_final/
// engine_threshold.json: registrations of n -> n points by the three paths) it wins or ties up to 7 splits (14k points:
// 0.385 against 0.416 ms on a LiDAR-like pair), ties at 10 and loses from 14 (uniform 28k: 1.03 against 0.93 ms).
// ICPMI_SMALL_MAX_SPLITS moves the limit (at most kSmallMaxSplits, what the kernel's LDS records hold).
constexpr int kSmallSplitsDefault = 8;

// when d_nrm/d_partials are given the resolve kernel also does k_reduce's work (one partial
// row per resolve workgroup: resolve_blocks(n) rows)
// Which resolve kernel: 0 = k_nn_resolve<16> (16 queries per wave, 64 per workgroup); 8 = k_nn_resolve4<8> (4 queries
// per wave, 32 per workgroup).  Measured (resolve + finish_step per pass, 100k targets): 8.8k / 12.5k / 25k queries
// 34 -> 25 / 37 -> 27 / 41 -> 36 us with the quarter-wave kernel, 50k / 100k queries 46 -> 52 / 63 -> 80 us (its 2-4x
// more partial rows and waves cost more than the shorter chains save).  32 queries per wave (k_nn_resolve<32>: all the
// waves of a C3 pass on the chip at once) lost too: 55.7 us against 48.7 at C3, the longer chain per wave costs more.
inline int resolve_waves(int n)
{
    return n <= 32768 ? 8 : 0;
}
inline int resolve_blocks(int n)
{
    const int w = resolve_waves(n);
    const int per = w > 0 ? 4 * w : kResolveWW * kResolveQ;
    return (n + per - 1) / per;
}
// workgroups of the stand-alone k_reduce family
inline int reduce_blocks(int cu_count, int n)
{
    return std::max(1, std::min(cu_count, (n + 255) / 256));
}
// All-pairs coarse pass on few units (filtered scans: 14 query blocks x 4 splits): 256-query units -- one
// 32-query tile per wave instead of two -- when even those fit the chip in one round (at most one unit per CU).
// The units' time is their waves' time there, so half the work per wave is a shorter pass; once the chip is full
// the 512-query unit amortises its staging and operand build over twice the results.
inline bool coarse_half_units(int cu_count, int n, int splits)
{
    const long units = (long)((n + kCoarseQueries - 1) / kCoarseQueries) * splits;
    return units <= (long)cu_count;
}

// ---- the facts a call's form is decided from ---------------------------------------------------------------------------
// (Everything the loop's conditions read.  m, normal_k and profile select no kernel today: the stages read them for sizes,
// the normals and the statistics, and a form that comes to depend on them finds them here.)
enum LoopRule { kRuleNone = 0, kRuleGate = 1, kRuleRobust = 2, kRuleGicp = 3 }; // plain / icp_gated.h / icp_robust.h / icp_gicp.h kernels

struct LoopFacts {
    int n = 0, m = 0;       // rows of the source (this rank's) and of the target
    int nn_engine = ICPMI_SEARCH_EXACT_F64; // what prepare_nn chose for the target: the engine, ...
    bool nn_pruned = false;                 // ... whether it is the culled one, ...
    int nn_splits = 0;                      // ... and the target's splits
    int cu_count = 256, normal_k = 20;
    bool comm = false;      // the context has a communicator or exchange callbacks
    LoopRule rule = kRuleNone;
    // plane-to-plane, small form allowed (ICPMI_GICP_FORM_SMALL; kRuleGicp only): at the small-cloud kernel's sizes the pass
    // runs k_icp_small_gicp.  Off, a plane-to-plane call has the general form at every size.
    bool gicp_small = false;
    int profile = 0;        // icpmi_options::profile
    // the environment switches, as capi.hip read them (ICPMI_SMALL, ICPMI_SMALL_MAX_SPLITS and ICPMI_FUSE_FINISH once per
    // process, the others at every call)
    bool sw_small = true;
    int sw_small_max_splits = kSmallSplitsDefault;
    bool sw_bounded = true, sw_reuse = true, sw_margin = true, sw_lean = true;
    int sw_lean_from = 0;   // ICPMI_NN_LEAN_FROM: 0 or k >= 2
    bool sw_fuse_finish = true;
    bool sw_cull_full = true; // ICPMI_NN_CULL_FULL, read at every call
    bool sw_solo = true;      // ICPMI_NN_SOLO, read at every call
    int sw_solo_from = 0;     // ICPMI_NN_SOLO_FROM: 0 or k >= 2
};

// (by the target alone: whether its Morton-ordered normals are worth keeping)
inline bool small_target(const LoopFacts &f)
{
    return f.sw_small && f.nn_engine == ICPMI_SEARCH_MFMA_BF16 && !f.nn_pruned && f.nn_splits <= f.sw_small_max_splits;
}

// Everything derived from the facts.  Field by field (DESIGN 4.7.4 has the table):
struct LoopPlan {
    LoopRule rule = kRuleNone;
    bool sharded = false;          // exchanges on, even for 1 rank
    bool fused = false;            // the resolve kernel also forms the normal-equation partial sums
    bool small = false;            // one kernel per iteration for the rows' work (icp_small.h), then k_finish_step
    bool pruned = false;           // the culled engine's loop: group lists, sorted rows
    bool sorted_rows_loop = false; // all-pairs engine, general kernels: the rows in Morton order
    bool sort_source = false;      // pruned || sorted_rows_loop: the source's bounding box, keys and sort are queued
    bool bounded = false;          // every pass searches behind a bound (nn_bounded.h)
    bool reuse = false;            // list reuse (RowBounds, kernels.h)
    bool margin = false;           // the match margin (list_reuse.h)
    bool lean_on = false;          // lean passes (list_reuse.h)
    int lean_from = 0;             // the test hook's first lean pass (0: by the counts)
    bool fused_tail = false;       // a loop pass ends in k_finish_step_transform* (single GPU, no rule, ICPMI_FUSE_FINISH on)
    int resolve_waves = 0;         // which resolve kernel (resolve_waves above)
    int rblocks = 0;               // partial rows a pass leaves
    bool sum_tree = false;         // ... first added in groups (k_sum_groups) ...
    int rblocks2 = 0;              // ... into this many rows behind them
    int fin_blocks = 0;            // rows the step kernels sum
    const char *error = nullptr;   // a refusal ("internal: ..."; a format that takes rblocks), or null
    bool cull_full = false;        // all-pairs engine: the two passes that list every row run over the box test's survivors
    bool solo_on = false;          // solo passes: a settled pass is one launch (k_finish_step_transform_solo, solo_pass.h)
    int solo_from = 0;             // the test hook's first solo tail (0: by the counts)
};

inline LoopPlan make_loop_plan(const LoopFacts &f)
{
    LoopPlan p;
    const int n = f.n;
    p.rule = f.rule;
    p.sharded = f.comm;
    // with the MFMA engine the resolve kernel also forms the normal-equation partial sums
    // (not under a gate: its general path searches first and tests the rows in k_reduce_gated)
    p.fused = f.nn_engine == ICPMI_SEARCH_MFMA_BF16 && f.rule == kRuleNone;
    // the sizes of the small-cloud kernel, whatever runs at them
    const bool small_sizes = !p.sharded && n <= kSmallMaxQueries && f.nn_splits <= f.sw_small_max_splits;
    // (plane-to-plane rows take the small-cloud form only where the caller allows it -- its sums are another order's,
    // icp_gicp.h -- and otherwise the gated general path at every size)
    p.small = small_sizes && n > 0 && small_target(f) && (f.rule != kRuleGicp || f.gicp_small);
    p.resolve_waves = resolve_waves(n);
    p.rblocks = p.small ? (n + kSmallQ - 1) / kSmallQ : (p.fused ? resolve_blocks(n) : reduce_blocks(f.cu_count, n));
    // very many partial rows (a resolve workgroup leaves one per 64 queries) are first added in groups of kSumGroup by a
    // kernel of their own (k_sum_groups, kernels.h): the step kernels then sum rblocks2 rows
    p.sum_tree = p.rblocks >= kSumTreeFrom;
    p.rblocks2 = p.sum_tree ? (p.rblocks + kSumGroup - 1) / kSumGroup : 0;
    p.fin_blocks = p.sum_tree ? p.rblocks2 : p.rblocks;
    // (k_sum_groups adds kNumSums columns, one short of a robust row's; a robust general pass leaves reduce_blocks() rows)
    if (f.rule == kRuleRobust && p.sum_tree && !p.small) p.error = "internal: a robust pass of %d partial rows";
    // (k_reduce_gicp and, where allowed, k_icp_small_gicp are the only kernels that form plane-to-plane sums: a plan that would
    // hand such a pass to the small-cloud kernel unasked, to a fused resolve or to k_sum_groups -- which a small pass never
    // launches, whatever sum_tree says -- is refused here, not launched with another rule's kernel or with none)
    if (f.rule == kRuleGicp && (p.small ? !f.gicp_small : (p.fused || p.sum_tree)))
        p.error = "internal: a plane-to-plane pass of %d partial rows has only the general form";

    // Pruned engine: the source is put in Morton order once (a rigid motion keeps neighbours
    // together), so that every block of kCoarseQueries consecutive rows of `cur` is a compact
    // blob whose bounding box can rule whole target splits out.  The order of the rows of
    // `cur` is internal: only sums over all rows leave the call.
    p.pruned = p.fused && f.nn_pruned && n > 0;
    // All-pairs engine, general kernels: the rows are taken in Morton order too (the order is internal here as well).  A
    // tile of 32 neighbouring rows has its matches in one or two splits, so the bounded pass's epilogue (nn_bounded.h)
    // finds nothing to list in the other 47 and leaves by its short path: with rows in the caller's order half of all
    // (tile, split) pairs listed something (k_nn_coarse_bounded 305 -> 295 us on C3, k_nn_resolve_bounded 29 -> 28).
    // (from 4,096 rows: below, the Morton sort of the rows costs a call more than its passes gain)
    // (not at the small-cloud kernel's sizes, where ICPMI_SMALL=0 puts the general kernels in its place: there they keep
    // its order of rows, hence its bits)
    // (and only against targets of more than a dozen splits: at 10 splits -- 18k x 20k points, six iterations -- the rows' sort is
    // 55 us of a 0.45 ms registration whose coarse pass is 5 us; profiles/r4_final/c2_20k/timeline.txt)
    constexpr int kSortRowsFromSplits = 12;
    p.sorted_rows_loop = p.fused && !p.pruned && !small_sizes && n >= 4096 && f.nn_splits > kSortRowsFromSplits;
    p.sort_source = p.pruned || p.sorted_rows_loop;

    // Bounded passes (nn_bounded.h): every kernel that moves the rows after a pass also leaves, per row, the exact distance
    // to the target it was just matched with -- the bound the next pass searches behind.
    // Round 4: the FIRST pass has a bound too -- the nearest of the sorted targets around each row's place in the target's
    // Morton order (k_nn_prebound1) stands in for the previous match -- so no pass of a registration keeps coarse minima:
    // the (row, split) buffer (6 B each: 2.9 GB at 1M x 1M) is not reserved by the loop at all.  Every general-path
    // loop of the MFMA engines is bounded now, whatever its row order (ICPMI_NN_BOUNDED=0: round 2's form for the
    // all-pairs engine, the A/B and fuzz reference; the culled engine has no other form).
    p.bounded = p.fused && !p.small && n > 0 && (p.pruned || f.sw_bounded);
    if (!p.error && p.pruned && !p.bounded) p.error = "internal: the culled engine needs the bounded resolve kernels";
    // List reuse (RowBounds, kernels.h), all-pairs engine: a row keeps its list of slots from pass to pass while its bound and
    // its drift from where the list was built show that a new list could hold nothing the kept one lacks, and the coarse
    // pass runs over the packed list of the rows that were listed again (k_row_list, queued behind the kernel that moves
    // the rows).  A call's first pass lists every row (k_nn_prebound1 marks its lists as not to be kept).  The culled engine
    // keeps its own form.
    p.reuse = p.bounded && !p.pruned && f.sw_reuse;
    // The match margin (list_reuse.h): rows whose kept match is certified as the unique nearest target are neither listed
    // nor scanned.  k_nn_resolve_bounded's loops only; the gated and robust loops keep the form before it.
    p.margin = p.reuse && f.rule == kRuleNone && p.resolve_waves == 0 && f.sw_margin;
    // Lean passes (list_reuse.h, "lean passes"): once the passes list no row, k_row_list and the coarse kernel
    // are no longer launched.  Single-GPU, ungated loops with list reuse, the fused finish kernel and a k_sum_groups launch,
    // whose extra workgroup tells the host how many rows each pass wanted listed (WantPublish, kernels.h); everywhere else
    // the launches are those of the form before.  The host learns the counts in the queue loop, two passes late, where it
    // waits for the progress word anyway: the launches are a function of the data, not of timing.
    p.fused_tail = !p.sharded && f.rule == kRuleNone && f.sw_fuse_finish;
    p.lean_on = p.reuse && p.fused_tail && p.sum_tree && f.sw_lean;
    p.lean_from = p.lean_on ? f.sw_lean_from : 0;
    // Culled full passes: a call's first two passes list every row -- the first has only k_nn_prebound1's
    // bound, the second follows lists that are not kept -- and evaluate all n x m pairs for it.  Over targets of the sizes
    // at which the 20-NN pass is culled (knn_culled, capi.hip) they run k_nn_coarse_groups on the (32-row tile, split) pairs
    // whose boxes are within the tile's largest listing radius instead: single GPU, no rule, list reuse on.  Every later
    // pass and every other kernel of the loop stays as it is.  ICPMI_NN_CULL_FULL=0: all pairs, the form before.
    // (Only where the rows are in Morton order: a tile of 32 rows in the caller's order spans the cloud, every pair survives
    // the box test and the lists are pure cost -- measured, sources of 1,000 to 4,000 unsorted rows against 30,000 and
    // 100,000 points: 0.525 -> 0.543, 0.789 -> 0.812 and 0.917 -> 0.935 ms a call of 9 iterations with the passes culled.)
    p.cull_full = p.reuse && p.sorted_rows_loop && !p.sharded && f.rule == kRuleNone && f.nn_splits > kKnnCullFromSplits &&
                  f.nn_splits <= kCullMaxSplits && n < kCullMaxRows && f.sw_cull_full;
    // Solo passes (solo_pass.h): once every row's match is certified, the kernel that ends a pass also forms
    // the next pass's terms and group sums for its own rows, and that pass launches nothing else.  Where lean passes and the
    // match margin are on, a workgroup of the moving kernel holds exactly the rows of one group sum (one row per thread, one
    // group row per workgroup: at most kFinishBlocksMax x kFinishThreads rows), and the stage brackets of profile level 2,
    // which want the three launches, are off.  ICPMI_NN_SOLO=0: the launches of the form before.
    p.solo_on = p.lean_on && p.margin && p.fin_blocks == finish_transform_blocks(n) && n <= kFinishBlocksMax * kFinishThreads &&
                f.profile < 2 && f.sw_solo;
    p.solo_from = p.solo_on ? f.sw_solo_from : 0;
    return p;
}

// ---- per pass (general kernels; the small-cloud pass has one form) ------------------------------------------------------
// sharded: step + pose update of this rank's rows in one launch behind the all-reduce (k_step_transform*)
inline bool fuse_step(const LoopPlan &p, int n, int final_pass) { return p.sharded && n > 0 && !final_pass; }
// single GPU: final sum + step + pose update of the rows in one launch (k_finish_step_transform*)
inline bool fuse_finish(const LoopPlan &p, int n, int final_pass) { return p.fused_tail && n > 0 && !final_pass; }

// Lean passes, the host's bookkeeping: whether the pass AFTER pass P (from 1) is queued lean, decided when pass P is
// queued from want[p - 1] = the rows pass p wanted listed, `known` of which the host has read.  The queue loop has read
// P - 2 of them by then and the two latest, want(P - 3) and want(P - 2), decide (lean_pass, list_reuse.h); a pass queued
// with fewer counts at hand is not lean.  `lean_from` (the test hook): every pass from that one on, whatever the counts.
inline bool lean_next(int P, int final_pass, int lean_from, const unsigned *want, int known)
{
    if (final_pass) return false;
    if (lean_from) return P + 1 >= lean_from;
    return P >= 6 && known >= P - 2 && lean_pass(P + 1, want[P - 4], want[P - 3]);
}

// Solo passes, the host's bookkeeping: whether the tail of pass P (from 1, never the post-loop pass) is the solo kernel,
// decided when pass P is queued from uncert[p - 1] = the rows pass p did not find certified, `known` of which the host has
// read (P - 2 by then, like the counts of lean_next).  It is when the two latest, uncert(P - 3) and uncert(P - 2), are 0:
// uncert(1) = uncert(2) = n, so never before pass 6, and a row that is not certified is not listed either, so the pass
// behind such a tail is lean by lean_next's own rule.  `solo_from` (the test hook): every tail from that pass on, whatever
// the counts; the queue loop then takes the passes behind them as lean.
inline bool solo_next(int P, int final_pass, int solo_from, const unsigned *uncert, int known)
{
    if (final_pass) return false;
    if (solo_from) return P >= solo_from;
    return P >= 6 && known >= P - 2 && uncert[P - 4] == 0u && uncert[P - 3] == 0u;
}

} // namespace icpmi
