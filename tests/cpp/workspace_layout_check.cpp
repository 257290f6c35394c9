// Host check of csrc/workspace_layout.h: every layout against the hand-written offsets and sizes it replaced in capi.hip,
// frozen below as they stood (sizes as literals, so that a changed constant or record in the header shows; addresses as
// integers from a fake base), offset for offset and byte for byte over the edges of every size they look at; then, per
// layout, that its members ascend, do not overlap, end within bytes() and are aligned as their readers need.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "workspace_layout.h"

using namespace icpmi;

namespace {

constexpr uintptr_t kBase = 0x10000; // (aligned to 64 bytes, as hipMalloc's are)
void *const kBasePtr = reinterpret_cast<void *>(kBase);

long failures = 0, checks = 0;
void expect(bool ok, const char *what, unsigned long long a, unsigned long long b = 0, unsigned long long c = 0)
{
    ++checks;
    if (ok) return;
    if (++failures <= 20) printf("FAIL %s: %llu %llu %llu\n", what, a, b, c);
}
template <class T> uintptr_t addr(const T *p) { return reinterpret_cast<uintptr_t>(p); }

// one member of a layout: where it starts, its bytes, the alignment its readers need
struct Member {
    const char *name;
    uintptr_t at;
    size_t bytes, align;
};
void check_members(const char *layout, const std::vector<Member> &ms, size_t total, unsigned long long arg)
{
    uintptr_t end = kBase;
    for (const Member &m : ms) {
        expect(m.at >= end, layout, arg, m.at, end);                   // ascending, no overlap
        expect(m.at % m.align == 0, m.name, arg, m.at, m.align);       // alignment
        end = m.at + m.bytes;
    }
    expect(end <= kBase + total, layout, arg, end - kBase, total);     // within bytes()
}

// ---- the formulae as capi.hip had them ------------------------------------------------------------------------------
// nn_list_bytes: kNnListRowBytes = sizeof(double) + 2 sizeof(float) + sizeof(int) + sizeof(unsigned) kNnEntCap + sizeof(RowList)
size_t ref_nn_list_bytes(int n)
{
    const size_t row = 8 + 2 * 4 + 4 + 4 * 8 + 32;
    return row * (size_t)n + 64 + 8 * (((size_t)n + 63) / 64) + 4 * ((size_t)n + 16) + 4 * 3 * 1024 + 64 + (32 + 8) * (size_t)n +
           8 * (((size_t)n + 63) / 64);
}
// nn_list_rows: the pointer walk, the two roundings done on the address
struct RefListRows {
    uintptr_t ub, ent, ubf, sqf, cnt, xb, mask, list, stat_rows, stat_cert, stat_searched, scan, cover, cert, end;
};
RefListRows ref_nn_list_rows(uintptr_t base, int n)
{
    RefListRows r;
    const size_t N = (size_t)n;
    r.ub = base;
    r.ent = r.ub + 8 * N;
    r.ubf = r.ent + 4 * (size_t)8 * N;
    r.sqf = r.ubf + 4 * N;
    r.cnt = r.sqf + 4 * N;
    r.xb = ((r.cnt + 4 * N) + 63) & ~(uintptr_t)63;
    r.mask = r.xb + 32 * N;
    r.list = r.mask + 8 * ((N + 63) / 64);
    r.stat_rows = r.list + 4 * (N + 16);
    r.stat_cert = r.stat_rows + 4 * 1024;
    r.stat_searched = r.stat_cert + 4 * 1024;
    r.scan = ((r.stat_searched + 4 * 1024) + 63) & ~(uintptr_t)63;
    r.cover = r.scan + 32 * N;
    r.cert = r.cover + 8 * N;
    r.end = r.cert + 8 * ((N + 63) / 64);
    return r;
}
// the group lists: `per` as reserve_group_lists, group_lists, group_stats and group_cnt_bytes each computed it
size_t ref_per_reserve(int splits) { return ((size_t)splits + 64 - 1) / 64 * 64; }
size_t ref_per_lists(int splits) { return ((size_t)splits + 64 - 1) / 64 * 64; }
size_t ref_per_stats(int splits) { return ((size_t)splits + 64 - 1) / 64 * 64; }
size_t ref_per_bytes(int splits) { return ((size_t)splits + 64 - 1) / 64 * 64; }
size_t ref_group_reserve(int splits) { return 4 * 2 * ref_per_reserve(splits) + 2 * 8 + 4 * 4; }
uintptr_t ref_group_set(uintptr_t base, int splits, int set) { return base + 4 * ((size_t)set * ref_per_lists(splits)); }
uintptr_t ref_group_stats(uintptr_t base, int splits) { return base + 4 * (2 * ref_per_stats(splits)); }
uintptr_t ref_group_work(uintptr_t base, int splits, int parity) { return ref_group_stats(base, splits) + 2 * 8 + 4 * (size_t)(parity & 1); }
size_t ref_group_cnt_bytes(int splits) { return 4 * 2 * ref_per_bytes(splits) + 2 * 8 + 4 * 4; }
long ref_items_cap(long groups) { return ((groups > 1 ? groups : 1) + 1) / 2 * 2; }
size_t ref_items_bytes(int splits, long cap) { return 4 * (size_t)splits * (size_t)cap + 16; }
// launch_knn: kListRowBytes and the carve of its two branches
constexpr long kRefListRowBytes = 8 + 2 * 4 + 4 + 4 * 32;
struct RefKnnRows {
    uintptr_t t_row, tf_row, sqf_row, cnt_row, ent_row;
};
RefKnnRows ref_knn_rows(uintptr_t base, long chunk)
{
    RefKnnRows r;
    r.t_row = base;
    r.tf_row = r.t_row + 8 * (size_t)chunk;
    r.sqf_row = r.tf_row + 4 * (size_t)chunk;
    r.cnt_row = r.sqf_row + 4 * (size_t)chunk;
    r.ent_row = r.cnt_row + 4 * (size_t)chunk;
    return r;
}
// settle_plan's reserve, solo_groups and solo_counts (kSumsStride 32, kFinishBlocksMax 128, SoloCounts 16 bytes)
size_t ref_partials_bytes(int rblocks, int rblocks2, bool solo)
{
    const size_t solo_bytes = solo ? 8 * 32 * (size_t)rblocks2 + 2 * 16 * 128 : 0;
    return 8 * 32 * ((size_t)rblocks + (size_t)rblocks2) + solo_bytes;
}
uintptr_t ref_solo_groups(uintptr_t base, int rblocks, int rblocks2, int area)
{
    return base + 8 * (32 * ((size_t)rblocks + (size_t)area * rblocks2));
}
uintptr_t ref_solo_counts(uintptr_t base, int rblocks, int rblocks2, int parity)
{
    return base + 8 * (32 * ((size_t)rblocks + 2 * (size_t)rblocks2)) + 16 * ((size_t)(parity & 1) * 128);
}

// ---- the checks -----------------------------------------------------------------------------------------------------
void check_misc()
{
    alignas(64) static char block[MiscBlock::kBytes];
    expect(MiscBlock::kBytes == 256, "misc bytes", MiscBlock::kBytes);
    expect(addr(MiscBlock::at<NnFrame>(block, MiscBlock::kTargetFrame)) == addr(block) + 0, "misc target frame", MiscBlock::kTargetFrame);
    expect(addr(MiscBlock::at<NnFrame>(block, MiscBlock::kSourceFrame)) == addr(block) + 64, "misc source frame", MiscBlock::kSourceFrame);
    expect(addr(MiscBlock::at<unsigned long long>(block, MiscBlock::kCounters)) == addr(block) + 128, "misc counters", MiscBlock::kCounters);
    expect(MiscBlock::kVoxelBox == 192, "misc voxel box", MiscBlock::kVoxelBox);
    expect(MiscBlock::kCounterBytes == 24 && sizeof(NnFrame) == 48, "misc sizes", MiscBlock::kCounterBytes, sizeof(NnFrame));
    expect(sizeof(RowList) == 32 && sizeof(RowScan) == 32 && sizeof(SoloCounts) == 16, "record sizes", sizeof(RowList), sizeof(RowScan),
           sizeof(SoloCounts));
}

void check_sort_planes(size_t count)
{
    const SortPlanes sp(kBasePtr, count);
    expect(addr(sp.keys_in) == kBase, "planes keys in", count);
    expect(addr(sp.keys_out) == kBase + 4 * count, "planes keys out", count);
    expect(addr(sp.vals_in) == kBase + 4 * (2 * count), "planes values in", count);
    expect(addr(sp.perm) == kBase + 4 * (3 * count), "planes perm", count);
    expect(sp.bytes == 16 * count && sp.bytes == SortPlanes(nullptr, count).bytes, "planes bytes", count, sp.bytes);
    check_members("planes", {{"keys_in", addr(sp.keys_in), 4 * count, 4}, {"keys_out", addr(sp.keys_out), 4 * count, 4},
                             {"vals_in", addr(sp.vals_in), 4 * count, 4}, {"perm", addr(sp.perm), 4 * count, 4}}, sp.bytes, count);
}

void check_bounded_rows(int n)
{
    const BoundedRows b(kBasePtr, (size_t)n);
    const RefListRows r = ref_nn_list_rows(kBase, n);
    const size_t N = (size_t)n, words = (N + 63) / 64;
    expect(addr(b.ub) == r.ub && addr(b.ent) == r.ent && addr(b.ubf) == r.ubf && addr(b.sqf) == r.sqf && addr(b.cnt) == r.cnt,
           "bounded rows, first part", N);
    expect(addr(b.xb) == r.xb && addr(b.mask) == r.mask && addr(b.list) == r.list, "bounded rows, list reuse", N, addr(b.xb), r.xb);
    expect(addr(b.stat_rows) == r.stat_rows && addr(b.stat_cert) == r.stat_cert && addr(b.stat_searched) == r.stat_searched,
           "bounded rows, statistics", N);
    expect(addr(b.scan) == r.scan && addr(b.cover) == r.cover && addr(b.cert) == r.cert, "bounded rows, margin", N, addr(b.scan), r.scan);
    // bytes(): never less than the walk's end, never more than nn_list_bytes, and the same from any 64-byte aligned base
    expect(kBase + b.bytes >= r.end && b.bytes <= ref_nn_list_bytes(n), "bounded rows bytes", N, b.bytes, ref_nn_list_bytes(n));
    expect(b.bytes == BoundedRows(nullptr, N).bytes, "bounded rows bytes by base", N);
    check_members("bounded rows",
                  {{"ub", addr(b.ub), 8 * N, 8}, {"ent", addr(b.ent), 4 * 8 * N, 8}, {"ubf", addr(b.ubf), 4 * N, 4}, {"sqf", addr(b.sqf), 4 * N, 4},
                   {"cnt", addr(b.cnt), 4 * N, 4}, {"xb", addr(b.xb), 32 * N, 64}, {"mask", addr(b.mask), 8 * words, 8},
                   {"list", addr(b.list), 4 * (N + 16), 4}, {"stat_rows", addr(b.stat_rows), 4 * 1024, 4},
                   {"stat_cert", addr(b.stat_cert), 4 * 1024, 4}, {"stat_searched", addr(b.stat_searched), 4 * 1024, 4},
                   {"scan", addr(b.scan), 32 * N, 64}, {"cover", addr(b.cover), 8 * N, 8}, {"cert", addr(b.cert), 8 * words, 8}},
                  b.bytes, N);
}

void check_knn_rows(long chunk)
{
    const KnnRows k(kBasePtr, (size_t)chunk);
    const RefKnnRows r = ref_knn_rows(kBase, chunk);
    const size_t C = (size_t)chunk;
    expect(addr(k.t_row) == r.t_row && addr(k.tf_row) == r.tf_row && addr(k.sqf_row) == r.sqf_row && addr(k.cnt_row) == r.cnt_row &&
               addr(k.ent_row) == r.ent_row, "k-NN rows", C);
    expect((long)KnnRows::kRowBytes == kRefListRowBytes && k.bytes == (size_t)kRefListRowBytes * C && k.bytes == KnnRows(nullptr, C).bytes,
           "k-NN rows bytes", C, k.bytes);
    check_members("k-NN rows", {{"t_row", addr(k.t_row), 8 * C, 8}, {"tf_row", addr(k.tf_row), 4 * C, 4}, {"sqf_row", addr(k.sqf_row), 4 * C, 4},
                                {"cnt_row", addr(k.cnt_row), 4 * C, 4}, {"ent_row", addr(k.ent_row), 4 * 32 * C, 4}}, k.bytes, C);
}

void check_group_counters(int splits)
{
    const GroupCounters g(kBasePtr, (size_t)splits);
    const size_t per = ref_per_reserve(splits);
    expect(addr(g.set[0]) == ref_group_set(kBase, splits, 0) && addr(g.set[1]) == ref_group_set(kBase, splits, 1), "group sets", splits);
    expect(addr(g.stats) == ref_group_stats(kBase, splits), "group statistics", splits);
    expect(addr(g.work[0]) == ref_group_work(kBase, splits, 0) && addr(g.work[1]) == ref_group_work(kBase, splits, 1), "group chunk counters", splits);
    expect(g.bytes == ref_group_reserve(splits) && g.bytes == ref_group_cnt_bytes(splits) && g.bytes == GroupCounters(nullptr, (size_t)splits).bytes,
           "group counters bytes", splits, g.bytes);
    check_members("group counters", {{"set 0", addr(g.set[0]), 4 * per, 4}, {"set 1", addr(g.set[1]), 4 * per, 4}, {"stats", addr(g.stats), 16, 8},
                                     {"work 0", addr(g.work[0]), 4, 4}, {"work 1", addr(g.work[1]), 4, 4}}, g.bytes, splits);
    for (long groups : {0l, 1l, 2l, 3l, 1024l, 1025l, (1l << 20) - 1}) {
        const long cap = GroupCounters::items_cap(groups);
        expect(cap == ref_items_cap(groups) && cap % 2 == 0 && cap >= groups, "group items cap", groups, cap);
        expect(GroupCounters::items_bytes((size_t)splits, cap) == ref_items_bytes(splits, cap), "group items bytes", splits, cap);
    }
}

void check_partial_rows(int rblocks, int rblocks2, bool solo)
{
    const PartialRows p(kBasePtr, rblocks, rblocks2, solo);
    const size_t R = (size_t)rblocks, R2 = (size_t)rblocks2;
    expect(addr(p.rows) == kBase, "partial rows", R);
    expect(addr(p.groups[0]) == kBase + 8 * 32 * R && addr(p.groups[0]) == ref_solo_groups(kBase, rblocks, rblocks2, 0), "group area 0", R, R2);
    expect(p.bytes == ref_partials_bytes(rblocks, rblocks2, solo) && p.bytes == PartialRows(nullptr, rblocks, rblocks2, solo).bytes,
           "partial rows bytes", R, R2, p.bytes);
    std::vector<Member> ms{{"rows", addr(p.rows), 8 * 32 * R, 8}, {"groups 0", addr(p.groups[0]), 8 * 32 * R2, 8}};
    if (solo) {
        expect(addr(p.groups[1]) == ref_solo_groups(kBase, rblocks, rblocks2, 1), "group area 1", R, R2);
        expect(addr(p.counts[0]) == ref_solo_counts(kBase, rblocks, rblocks2, 0) && addr(p.counts[1]) == ref_solo_counts(kBase, rblocks, rblocks2, 1) &&
                   addr(p.counts[0]) == ref_solo_counts(kBase, rblocks, rblocks2, 2), "solo counts", R, R2);
        ms.push_back({"groups 1", addr(p.groups[1]), 8 * 32 * R2, 8});
        ms.push_back({"counts 0", addr(p.counts[0]), 16 * 128, 4});
        ms.push_back({"counts 1", addr(p.counts[1]), 16 * 128, 4});
    }
    check_members("partial rows", ms, p.bytes, R);
}

void check_rings()
{
    expect(kFlagRing == 8 && ProgressRings::kProgressWords == 8 && ProgressRings::kCountWords == 16, "ring sizes", kFlagRing);
    for (int slot = 0; slot < kFlagRing; ++slot) {
        expect(ProgressRings::wanted(slot) == slot && ProgressRings::uncertified(slot) == 8 + slot, "ring slots", slot);
        expect(ProgressRings::uncertified(slot) < ProgressRings::kCountWords && ProgressRings::wanted(slot) < ProgressRings::uncertified(0),
               "ring slots apart", slot);
    }
}

} // namespace

int main()
{
    const int sizes[] = {1, 31, 32, 63, 64, 65, 511, 512, 513, 4095, 4096, 32768, 32769, 100000, (1 << 25) - 1};
    check_misc();
    check_rings();
    for (int n : sizes) {
        check_bounded_rows(n);
        check_sort_planes((size_t)n);
        check_knn_rows(n);
        check_knn_rows(((long)n + 511) / 512 * 512);
    }
    check_sort_planes(((size_t)1 << 27) - 1);
    for (int splits : {1, 12, 13, 63, 64, 65, 3071, 3072}) check_group_counters(splits);
    // the partial rows of the plans of the sizes where the loop changes form, on the all-pairs engine over a large target (the
    // resolve's rows, summed in groups from 65,536 rows on, solo passes where the plan has them) and over a small one (the
    // small-cloud kernel's rows), each with and without the solo areas
    int solo_plans = 0;
    for (int n : {1, 32768, 32769, 65536, 100000, 131072})
        for (int splits : {4, 49})
            for (bool sw_solo : {false, true}) {
                LoopFacts f;
                f.n = n, f.m = splits * 2048, f.nn_engine = ICPMI_SEARCH_MFMA_BF16, f.nn_splits = splits, f.sw_solo = sw_solo;
                const LoopPlan p = make_loop_plan(f);
                solo_plans += p.solo_on;
                check_partial_rows(p.rblocks, p.rblocks2, p.solo_on);
                check_partial_rows(p.rblocks, p.rblocks2, !p.solo_on);
            }
    expect(solo_plans > 0, "a plan with solo passes among them", solo_plans);
    if (failures) {
        printf("%ld of %ld checks failed\n", failures, checks);
        return 1;
    }
    printf("ok %ld checks\n", checks);
    return 0;
}
