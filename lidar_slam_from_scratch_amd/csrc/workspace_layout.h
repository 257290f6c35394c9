// workspace_layout.h -- where things lie inside the context's shared device buffers, for host and device compilers alike:
// no HIP in here, no getenv.  Each buffer that holds more than one thing has ONE definition below, a small value type
// that walks the allocation once (Carve) and leaves typed pointers and the bytes the walk took; capi.hip sizes the
// buffer and addresses it through the same type, and tests/cpp/workspace_layout_check.cpp holds every walk to the
// hand-written offsets it replaced.  The plain records and the sizes a layout depends on are defined here, once; the
// kernels use the same names.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "loop_plan.h"

namespace icpmi {

// ---- sizes the kernels and the layouts share -----------------------------------------------------------------------
constexpr int kSumsStride = 32;        // doubles per partial row of normal-equation sums (kNumSums of them used; kernels.h)
constexpr int kNnEntCap = 8;           // list words per row of the bounded 1-NN pass (nn_mfma.h, nn_bounded.h)
constexpr int kKnnEntCap = 32;         // list words per row of the k-NN lists (knn_lists.h)
constexpr int kRowListHead = 16;       // words in front of the packed list of rows (the rows start on a 64-byte line)
constexpr int kReuseStatPasses = 1024; // list reuse's per-pass statistics (passes beyond overwrite the last entry)
constexpr int kGrpCntPad = 64;         // a set of per-split group counters is padded to a multiple of this many words
constexpr int kFlagRing = 8;           // slots of the host-mapped rings the device reports a pass's progress and counts in

// ---- the plain records a layout needs the size of ------------------------------------------------------------------
struct NnFrame {     // bounding box of a whole cloud (Morton quantisation; nn_mfma.h)
    double lo[3], hi[3];
};
struct RowList {     // list reuse (RowBounds, kernels.h)
    double x, y, z; // where the row's list was built
    double r;       // its listing radius R_b (NaN: the list is not to be kept, e.g. a call's first pass)
};
struct RowScan {     // the match margin (RowBounds, kernels.h)
    double x, y, z; // where the resolve last scanned the row's listed slots
    double g;       // every target but that scan's winner is at least g away from there (NaN: nothing is known)
};
struct SoloCounts {  // solo passes (solo_pass.h)
    unsigned want, uncert, searched, pad; // of one workgroup's rows: listed again, not certified, searched by the solo kernel
};

// One walk through an allocation: c(p, count) points p at the next `count` elements of its type.  Offsets are counted in
// bytes from the base and the pointer is formed last, so a walk from a null base gives the plain offsets (and the size to
// reserve) without any pointer arithmetic; all of it in size_t.  `align` rounds the OFFSET up: the same address as rounding
// the pointer for any base aligned to as much, which hipMalloc guarantees for the 64 bytes used below.
struct Carve {
    uintptr_t base;
    size_t off = 0;
    explicit Carve(const void *p) : base(reinterpret_cast<uintptr_t>(p)) {}
    template <class T> Carve &operator()(T *&p, size_t count)
    {
        p = reinterpret_cast<T *>(base + off);
        off += sizeof(T) * count;
        return *this;
    }
    Carve &align(size_t a) { return off = (off + a - 1) / a * a, *this; }
};

// ---- nn_misc: the target's frame, the source's, the resolve's three counters (rows rechecked, rows that fell back,
// blocks culled) and the voxel filter's box (an NnFrame by another name: voxel.h), each on a 64-byte line of its own -----
struct MiscBlock {
    static constexpr size_t kTargetFrame = 0, kSourceFrame = 64, kCounters = 128, kVoxelBox = 192, kBytes = 256;
    static constexpr size_t kCounterBytes = 3 * sizeof(unsigned long long);
    template <class T> static T *at(void *base, size_t offset) { return reinterpret_cast<T *>(static_cast<char *>(base) + offset); }
};
static_assert(MiscBlock::kTargetFrame + sizeof(NnFrame) <= MiscBlock::kSourceFrame && MiscBlock::kSourceFrame + sizeof(NnFrame) <= MiscBlock::kCounters &&
                  MiscBlock::kCounters + MiscBlock::kCounterBytes <= MiscBlock::kVoxelBox && MiscBlock::kVoxelBox + sizeof(NnFrame) <= MiscBlock::kBytes,
              "the four parts of the misc block lie apart");

// ---- sort_keys (the target's m rows), src_sort (the source's n): the four planes of one Morton sort -- keys in, sorted
// keys, values in, the permutation --------------------------------------------------------------------------------------
struct SortPlanes {
    unsigned *keys_in, *keys_out, *vals_in, *perm;
    size_t bytes;
    SortPlanes(const void *base, size_t count)
    {
        bytes = Carve(base)(keys_in, count)(keys_out, count)(vals_in, count)(perm, count).off;
    }
};

// ---- nn_lists: the bounded pass's per-row arrays (bound, list words, the coarse pass's radius^2 and its root, list
// length); on a 64-byte line list reuse's records, its word per 64 rows, its packed list of rows (kRowListHead words in
// front) and the per-pass statistics (profiling: rows listed, rows certified by the match margin, rows the solo kernel
// searched); on a 64-byte line the match margin's records, covers and word per 64 rows (RowBounds, kernels.h) -----------
struct BoundedRows {
    double *ub, *cover;
    unsigned *ent, *stat_rows, *stat_cert, *stat_searched; // (ent: 8-byte aligned, read two words at a time)
    float *ubf, *sqf;
    int *cnt, *list;
    RowList *xb;
    RowScan *scan;
    unsigned long long *mask, *cert;
    size_t bytes;
    explicit BoundedRows(const void *base = nullptr, size_t n = 0)
    {
        Carve c(base);
        c(ub, n)(ent, kNnEntCap * n)(ubf, n)(sqf, n)(cnt, n).align(64);
        c(xb, n)(mask, (n + 63) / 64)(list, n + kRowListHead);
        c(stat_rows, kReuseStatPasses)(stat_cert, kReuseStatPasses)(stat_searched, kReuseStatPasses).align(64);
        bytes = c(scan, n)(cover, n)(cert, (n + 63) / 64).off;
    }
};

// ---- slotmin as the k-NN lists of a chunk of rows (knn_lists.h): bound, its fp32 forms, list length, kKnnEntCap words --
struct KnnRows {
    static constexpr size_t kRowBytes = sizeof(double) + 2 * sizeof(float) + sizeof(int) + sizeof(unsigned) * kKnnEntCap;
    double *t_row;
    float *tf_row, *sqf_row;
    int *cnt_row;
    unsigned *ent_row;
    size_t bytes; // kRowBytes a row
    KnnRows(const void *base, size_t chunk)
    {
        bytes = Carve(base)(t_row, chunk)(tf_row, chunk)(sqf_row, chunk)(cnt_row, chunk)(ent_row, kKnnEntCap * chunk).off;
    }
};

// ---- grp_cnt: two alternating sets of per-split counters (a pass reads one and clears the other), two statistics
// words behind them, then four words of which the first two are the coarse kernel's chunk counters, one per parity of the
// pass (nn_culled.h).  grp_items: per split a list of `cap` groups -- even, the coarse kernel reads a wave's two entries as
// one 8-byte word -------------------------------------------------------------------------------------------------------
struct GroupCounters {
    unsigned *set[2], *work[2];
    unsigned long long *stats;
    size_t bytes;
    GroupCounters(const void *base, size_t splits)
    {
        const size_t per = (splits + kGrpCntPad - 1) / kGrpCntPad * kGrpCntPad;
        bytes = Carve(base)(set[0], per)(set[1], per)(stats, 2)(work[0], 1)(work[1], 3).off;
    }
    static long items_cap(long groups) { return ((groups > 1 ? groups : 1) + 1) / 2 * 2; }
    static size_t items_bytes(size_t splits, long cap) { return sizeof(unsigned) * splits * (size_t)cap + 16; }
};

// ---- partials: a pass's partial rows, their sums in groups behind them and, with solo passes, a second area of group
// rows and two sets of per-workgroup counts, by parity of the pass (solo_pass.h; without them neither reserved nor used) --
struct PartialRows {
    double *rows, *groups[2];
    SoloCounts *counts[2];
    size_t bytes;
    explicit PartialRows(const void *base = nullptr, int rblocks = 0, int rblocks2 = 0, bool solo = false)
    {
        Carve c(base);
        bytes = c(rows, kSumsStride * (size_t)rblocks)(groups[0], kSumsStride * (size_t)rblocks2).off;
        c(groups[1], kSumsStride * (size_t)rblocks2)(counts[0], kFinishBlocksMax)(counts[1], kFinishBlocksMax);
        if (solo) bytes = c.off;
    }
};

// ---- the host-mapped rings: kFlagRing progress words; of the count words the first kFlagRing are "rows wanted listed",
// the next as many "rows not certified", both at the slot of the pass's progress word -----------------------------------
struct ProgressRings {
    static constexpr int kProgressWords = kFlagRing, kCountWords = 2 * kFlagRing;
    static constexpr int wanted(int slot) { return slot; }
    static constexpr int uncertified(int slot) { return kProgressWords + slot; }
};

} // namespace icpmi
