// capi.hip -- host side of libicp_mi355x.so: the C ABI declared in include/icp_mi355x.h.
//
// Orchestrates the kernels of kernels.h on one HIP stream per context.  The ICP loop
// (icp.hpp:181-232) runs device-side: the error, both convergence tests, the 6x6 solve
// and the pose accumulation are done by k_finish_step, and once the loop has ended the
// remaining queued kernels return at their first instruction.  The host only looks at a
// 4-byte flag, two iterations behind the launch front, to stop queueing.
//
// There is no CPU fallback anywhere in this file.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <chrono>

#include <dirent.h>
#include <dlfcn.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <sched.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/icp_mi355x.h"
#include "loop_plan.h"
#include "workspace_layout.h"
#include "kernels.h"
#include "nn_mfma.h"
#include "icp_small.h"
#include "icp_gated.h"
#include "icp_robust.h"
#include "icp_gicp.h"
#include "knn_lists.h"
#include "nn_bounded.h"
#include "solo_pass.h"
#include "nn_culled.h"
#include "voxel.h"
#include "scan_context.h"
#include "occupancy.h"
#include "global_map.h"
#include "raycast.h"
#include "raycount.h"
#include "live_plane.h"
#include "live_counts.h"
#include "ground.h"
#include "static_map.h"
#include "deskew.h"
#include "loop_store.h"
#include "pose_graph.h"
#include "pose_graph_loss.h"
#include "pose_graph_info.h"
#include "pose_graph_marginals.h"
#include "pose_graph_marginals_host.h"
#include "local_map.h"

using namespace icpmi;

namespace icpmi {
hipError_t sort_pairs_u32(void *temp, size_t *temp_bytes, const unsigned *keys_in, unsigned *keys_out,
                          const unsigned *vals_in, unsigned *vals_out, unsigned n, hipStream_t stream);
hipError_t sort_pairs_u64(void *temp, size_t *temp_bytes, const unsigned long long *keys_in,
                          unsigned long long *keys_out, const unsigned *vals_in, unsigned *vals_out,
                          unsigned n, hipStream_t stream);
hipError_t sort_pairs_u64_all(void *temp, size_t *temp_bytes, const unsigned long long *keys_in,
                              unsigned long long *keys_out, const unsigned *vals_in, unsigned *vals_out,
                              unsigned n, hipStream_t stream);
hipError_t run_lengths_u64(void *temp, size_t *temp_bytes, const unsigned long long *keys, unsigned n,
                           unsigned long long *unique_out, unsigned *counts_out, unsigned *runs_out,
                           hipStream_t stream);
hipError_t exclusive_sum_u32(void *temp, size_t *temp_bytes, const unsigned *in, unsigned *out, unsigned n,
                             hipStream_t stream);
hipError_t sort_keys_u64(void *temp, size_t *temp_bytes, const unsigned long long *keys_in,
                         unsigned long long *keys_out, unsigned n, hipStream_t stream);
hipError_t merge_keys_u64(void *temp, size_t *temp_bytes, const unsigned long long *a, const unsigned long long *b,
                          unsigned long long *out, unsigned na, unsigned nb, hipStream_t stream);
}

namespace {

// last error of calls that have no context (icpmi_create, icpmi_load_cloud): per thread, so that
// contexts created on different threads (slam_icp_adapter.hpp holds one per thread) do not race
thread_local std::string g_create_error;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct EventPair {
    hipEvent_t a, b;
    int stage;
};

enum Stage { ST_NN = 0, ST_REDUCE = 1, ST_TRANSFORM = 2, ST_NORMALS = 3, ST_TOTAL = 4, ST_LOOP = 5, ST_SETUP = 6, ST_COARSE = 7, ST_EXCHANGE = 8 };

// roctx ranges around the stages of a call (SURVEY section 5 "Tracing"): visible to
// `rocprofv3 --marker-trace`.  The library is looked up at run time (the rocprofiler-sdk's roctx
// first, the older libroctx64 otherwise) and a missing one only means no ranges.  Costs two indirect calls per stage when nothing listens.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        // rocprofv3 traces the rocprofiler-sdk's roctx; the older libroctx64 is what roctracer-era tools see
        const char *names[] = {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "/opt/rocm/lib/librocprofiler-sdk-roctx.so.1",
                               "libroctx64.so", "libroctx64.so.4", "/opt/rocm/lib/libroctx64.so.4"};
        for (const char *nm : names) {
            void *lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
            if (!lib) continue;
            push = reinterpret_cast<int (*)(const char *)>(dlsym(lib, "roctxRangePushA"));
            pop = reinterpret_cast<int (*)()>(dlsym(lib, "roctxRangePop"));
            if (push && pop) return;
            push = nullptr;
            pop = nullptr;
        }
    }
};
const Roctx &roctx()
{
    static Roctx r;
    return r;
}
struct Range { // RAII: one roctx range
    explicit Range(const char *name) { if (roctx().push) roctx().push(name); }
    ~Range() { if (roctx().pop) roctx().pop(); }
    Range(const Range &) = delete;
    Range &operator=(const Range &) = delete;
};

struct Rccl {
    void *lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    decltype(&ncclCommUserRank) CommUserRank = nullptr;
    decltype(&ncclCommCuDevice) CommCuDevice = nullptr;
};

} // namespace

// A KITTI .bin on its way from disk to the device while the caller's thread runs the previous frame
// (icpmi_stream_prefetch_file): a worker thread reads it into pinned memory (~140 us for a 1.8 MB scan
// out of the page cache, nothing of the GPU's), copies it over on a stream of its own (the copy engine
// runs beside the compute of the frame in flight; on the context's stream it would queue behind it) and
// widens it there (k_widen_f32).  Two device slots: the push of a frame works out of one while the next
// frame lands in the other.
struct FilePrefetch {
    std::thread worker;
    std::mutex mu;
    std::condition_variable cv;
    std::string want;         // path being read (valid while `busy`)
    std::string ready[2];     // per device slot: the path whose points wait there for the push of that path
    void *h_buf[2] = {nullptr, nullptr};   // pinned staging, one per device slot (the worker's alone)
    size_t h_cap[2] = {0, 0};
    // The worker does not wait for its own GPU work: it records `filled[slot]` behind the copies, the widening and the
    // filter and announces the file; the push of that file waits for the event and reads the filter's outcome (number
    // of voxels, range flag) from pinned memory.  The worker's host time per file is then the read alone.
    hipEvent_t filled[2] = {nullptr, nullptr};
    unsigned *h_runs = nullptr;            // pinned: per slot {voxels, flag}
    bool pending[2] = {false, false};      // announced, event not yet waited for
    bool pend_filtered[2] = {false, false};
    double pend_voxel[2] = {0.0, 0.0};
    void *d_f32[2] = {nullptr, nullptr};   // device: the float32 records as read
    double *d_raw[2] = {nullptr, nullptr}; // device: N x 3 fp64 raw points
    size_t d_cap[2] = {0, 0};              // records each slot holds
    int64_t ready_n[2] = {0, 0};
    unsigned long long ready_seq[2] = {0, 0}, seq = 0; // which pending file is the older one
    hipEvent_t slot_done[2] = {nullptr, nullptr};      // recorded on the context's stream behind the push that read a slot
    bool slot_used[2] = {false, false};                // ... if any push has read it yet
    int taking = -1;                                   // the slot a push is reading right now: never the worker's choice
    hipStream_t stream = nullptr;
    bool busy = false, quit = false;
    int device = 0;
    // ... and filtered there too (voxel_filter_core on the worker's stream, with working memory of its own), with the
    // voxel size of the stream's last push: the push of the file then starts at the registration
    double voxel_hint = 0.0;               // 0: no push yet, the worker stops after the widening
    DevBuf filtered[2];                    // per slot: the filtered scan ...
    int64_t filtered_n[2] = {0, 0};        // ... its rows ...
    double filtered_voxel[2] = {0.0, 0.0}; // ... and the voxel size it was made with (0: not filtered)
    DevBuf sc_bbox, sc_box, sc_keys, sc_vals, sc_tmp;
    // where the worker's time goes (ICPMI_PREFETCH_STATS=1: printed to stderr when the context is destroyed)
    double t_wait = 0, t_read = 0, t_upload = 0, t_filter = 0;
    long files = 0;
};

// One more registration beside the caller's (icpmi_align_batch): a helper context -- stream, workspace -- and the
// host thread that drives it (align_device spins on the device's progress words, so every concurrent
// registration needs a host thread); the thread is kept between calls (starting one costs tens of microseconds,
// a tenth of a small registration).
struct BatchWorker {
    icpmi_ctx *helper = nullptr;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<void()> job;
    bool has_job = false, done = false, quit = false;
};

// What defines a prepared target (prepare_nn, prepare_target): its search structure, its normals, what the engine chose for
// it and whose preparation it is.  A context holds one; adopt_target hands a helper context's over whole.
struct PreparedTarget {
    DevBuf bpack, nn_misc;                    // MFMA engine: operands; frames + counters (MiscBlock, workspace_layout.h)
    DevBuf sort_keys, tgt_sorted, frames;     // Morton pre-pass: the sort's planes (SortPlanes), sorted copy, split frames
    DevBuf nrm, nrm_sorted;                   // the normals by point; small-cloud kernel: in Morton order (SoA, stride nn_ms)
    int nn_engine = ICPMI_SEARCH_EXACT_F64;   // engine prepared for the current target
    bool nn_pruned = false;                   // the culled engine (ICPMI_SEARCH_MFMA_PRUNED; AUTO on large targets)
    int nn_splits = 0;
    int nn_ms = 0;                            // component stride of the SoA sorted target
    int m = 0;                                // its rows (MFMA engines)
    // the target whose search structure and normals the buffers currently hold (prepare_target):
    // icpmi_stream_push prepares the NEXT frame's target while the caller is still busy with this frame's result
    const double *prep_tgt = nullptr;
    int prep_m = 0, prep_engine = 0;
    bool prep_valid = false;

    const unsigned *perm() const { return SortPlanes(sort_keys.p, (size_t)m).perm; }
    const unsigned *sorted_keys() const { return SortPlanes(sort_keys.p, (size_t)m).keys_out; }
    NnFrame *frame() const { return MiscBlock::at<NnFrame>(nn_misc.p, MiscBlock::kTargetFrame); }
    NnFrame *source_frame() const { return MiscBlock::at<NnFrame>(nn_misc.p, MiscBlock::kSourceFrame); }
    unsigned long long *counters() const { return MiscBlock::at<unsigned long long>(nn_misc.p, MiscBlock::kCounters); }
    const SplitFrame *split_frames() const { return (const SplitFrame *)frames.p; }
    const double *sorted() const { return (const double *)tgt_sorted.p; }
    const uint4 *operands() const { return (const uint4 *)bpack.p; }
};
static_assert(sizeof(VoxelBox) == sizeof(NnFrame), "the voxel filter's box takes an NnFrame's place in the misc block");

struct icpmi_ctx {
    icpmi_options opt;
    hipStream_t stream = nullptr;
    std::string err;
    int cu_count = 256;

    PreparedTarget tgt;
    DevBuf cur, idx, part_d2, part_idx, partials, history, stage_a, stage_b, stage_c, d2out;
    DevBuf knn_idx, slotmin, fb_list;         // k-NN lists, slot minima, rows for the exact fallback
    DevBuf nn_lists;                          // bounded 1-NN pass: per row bound, threshold, count, listed columns (nn_bounded.h)
    DevBuf src_nrm;                           // plane-to-plane ICP: the source's normals, in the caller's row order (icp_gicp.h)
    DevBuf vox_keys, vox_vals, vox_out;             // voxel filter: 64-bit keys (in/out/unique), values + run data, result
    DevBuf stream_prev, stream_cur, f32_stage;      // odometry stream: previous / current filtered scan; float32 upload staging
    int64_t stream_prev_n = -1;                     // rows of stream_prev (-1: no frame yet)
    int64_t stream_cur_n = 0;                       // rows of stream_cur while a push is registering it
    bool stream_robust_on = false;                  // icpmi_stream_set_robust: the pushes register under stream_robust
    icpmi_robust stream_robust{};
    icpmi_robust_info stream_robust_info{};         // icpmi_stream_last_robust: of the last push
    bool stream_deskew_on = false;                  // icpmi_stream_set_deskew: the pushes deskew the raw scan under stream_deskew first
    icpmi_deskew_config stream_deskew{};
    DevBuf deskew_raw, deskew_times;                // the deskewed raw scan of a push; icpmi_deskew's times on the device
    DevBuf grid_set, grid_in, grid_out, grid_cnt, world; // occupancy grid: the set (sorted unique keys), {set, new keys}, sorted, run data; world points
    int64_t grid_n = 0;                             // cells in grid_set
    unsigned *h_grid = nullptr;                     // pinned: the set's size on its way back
    unsigned long long *h_cnt = nullptr;            // pinned: the resolve's counters on their way back (profiling)
    std::vector<unsigned> reuse_rows, reuse_blocks; // profiling: per pass of the last registration, rows listed and workgroup columns run
    std::vector<unsigned> margin_rows;              // ... and rows certified by the match margin (empty where it was off)
    FilePrefetch *prefetch = nullptr;               // worker reading the next frame file (icpmi_stream_prefetch_file)
    hipEvent_t result_ready = nullptr;              // recorded behind a call's result copies (stream path)
    bool trailing_work = false;                     // a push returned with the next target's preparation still queued
    // odometry stream: the NEXT target's search structure and normals are built on a stream and workspace of their
    // own (a helper context) BESIDE the registration of the current frame, and adopted by swapping buffers
    icpmi_ctx *prep_helper = nullptr;
    hipEvent_t prep_done = nullptr;                 // recorded on the helper's stream behind a preparation
    hipEvent_t scan_ready = nullptr;                // recorded on this context's stream behind the filter of the scan to prepare
    bool helper_busy = false;                       // a preparation is queued on the helper and nothing has waited for it yet
    // where the calling thread's time goes in the frame stream (ICPMI_STREAM_STATS=1: printed when the context is destroyed)
    double t_push = 0, t_wait_file = 0, t_prep_queue = 0, t_align = 0, t_gpu_span = 0;
    long pushes = 0;
    DevBuf sort_tmp, coarse, bbox_part;       // the sorts' working memory; MFMA engine: coarse minima; bounding-box partials
    DevBuf src_sort;                          // Morton order of the source rows (the loop's internal order; SortPlanes)
    // the rows the last registration left in cur / idx (icpmi_debug_loop_rows): their count (-1: no registration has
    // completed since), whether idx holds the last pass's matches (not after the small-cloud kernel, which keeps them in
    // registers, nor after a nearest_batch call, which reuses the buffer), whether the rows were Morton-sorted (src_sort)
    int64_t loop_rows = -1;
    bool loop_idx_valid = false, loop_sorted = false;

    DevBuf grp_cnt, grp_items;                // culled engine: per target split the list of 64-row groups within reach (nn_culled.h)
    int grp_cap = 0;                          // groups a split's list in grp_items can hold
    IcpState *d_state = nullptr;   // two of them (align_device alternates in the sharded loop)
    IcpState *h_state = nullptr;   // pinned
    double *h_hist = nullptr;      // pinned: the error history of the last call
    size_t h_hist_cap = 0;
    void *h_file = nullptr;        // pinned: a frame file on its way to the device (icpmi_stream_push_file)
    size_t h_file_cap = 0;
    int32_t *h_flags = nullptr;    // host-mapped ring: (iteration + 1) * 2 + done, written by the device
    int32_t *d_flags = nullptr;    // the same words through the device's address space
    unsigned long long *h_want = nullptr; // host-mapped ring beside it: (iteration + 1) << 32 | rows the pass wanted listed
    unsigned long long *d_want = nullptr; // (lean passes: list_reuse.h; written by k_sum_groups)
                                          // (solo passes: a second ring behind it, the rows the pass did not find certified)
    unsigned *h_stat = nullptr;    // pinned: list reuse's per-pass statistics on their way back (profiling)
    // icpmi_last_normal_matrix: the sums of the pass that produced final_error of the last registration on this context,
    // taken from the state that came back behind its one wait (LoopRun::fill_result); nm_count: the problems of the last
    // batch this context led (problem k >= 1 ran on helper k - 1, which holds its record), 1 after a single call
    icpmi_normal_matrix nm{};
    bool nm_valid = false;
    int nm_count = 1;

    // profiling
    std::vector<EventPair> ev_pool;
    size_t ev_used = 0;
    unsigned coarse_seen = 0;      // k_nn_coarse launches since the context was made (profile 1 samples them)
    unsigned exchange_seen = 0;    // ... and the per-pass all-reduces of a sharded run
    icpmi_profile prof;

    // multi-GPU
    Rccl rccl;
    ncclComm_t comm = nullptr;
    int n_ranks = 1, rank = 0;
    icpmi_allreduce_fn cb_allreduce = nullptr;
    icpmi_allgather_fn cb_allgather = nullptr;
    void *cb_user = nullptr;
    std::vector<double> cb_host;
    std::vector<BatchWorker *> helpers; // icpmi_align_batch: one more stream + workspace + host thread per concurrent registration
};

namespace {

constexpr int kLag = 2; // (the rings of kFlagRing slots: ProgressRings, workspace_layout.h)

int fail(icpmi_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    else g_create_error = buf;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                    \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(ctx, ICPMI_ERR_HIP, "%s failed: %s (%s:%d)", #expr,                   \
                        hipGetErrorString(e_), __FILE__, __LINE__);                           \
    } while (0)

// grow-only with slack: odometry clouds vary frame to frame.  No context: also what the prefetch worker calls.
hipError_t reserve_raw(DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return hipSuccess;
    hipError_t e;
    if (b.p && (e = hipFree(b.p)) != hipSuccess) return e;
    b.p = nullptr;
    b.cap = 0;
    size_t want = std::max(bytes, (size_t)4096);
    want = want + want / 4;
    if ((e = hipMalloc(&b.p, want)) != hipSuccess) return e;
    b.cap = want;
    return hipSuccess;
}
int reserve(icpmi_ctx *ctx, DevBuf &b, size_t bytes)
{
    HIP_TRY(ctx, reserve_raw(b, bytes));
    return ICPMI_OK;
}

void release(DevBuf &b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

// ---- profiling helpers ----------------------------------------------------------------
struct StageTimer {
    icpmi_ctx *ctx;
    long slot = -1; // index, not pointer: the pool may reallocate while an outer timer is open
    StageTimer(icpmi_ctx *c, int stage) : ctx(c)
    {
        // profile 1: only the dominant kernel and the call/loop brackets (3 event pairs per
        // iteration would already cost ~10 us of stream time); profile >= 2: every stage
        if (!ctx->opt.profile) return;
        if (ctx->opt.profile == 1 && stage != ST_COARSE && stage != ST_TOTAL && stage != ST_LOOP && stage != ST_EXCHANGE) return;
        // profile 1 brackets the dominant kernel on every 4th launch only: an event pair costs the
        // stream ~5 us, and on every launch that was 2.2 % of a C3 call (scripts/event_overhead.py);
        // the average over the sampled launches is the same number
        if (ctx->opt.profile == 1 && stage == ST_COARSE && (ctx->coarse_seen++ & 3) != 0) return;
        if (ctx->opt.profile == 1 && stage == ST_EXCHANGE && (ctx->exchange_seen++ & 3) != 0) return; // (the same sampling)
        if (ctx->ev_used == ctx->ev_pool.size()) {
            EventPair p;
            if (hipEventCreate(&p.a) != hipSuccess) return;
            if (hipEventCreate(&p.b) != hipSuccess) {
                (void)hipEventDestroy(p.a);
                return;
            }
            p.stage = stage;
            ctx->ev_pool.push_back(p);
        }
        slot = (long)ctx->ev_used++;
        ctx->ev_pool[slot].stage = stage;
        (void)hipEventRecord(ctx->ev_pool[slot].a, ctx->stream);
    }
    ~StageTimer()
    {
        if (slot >= 0) (void)hipEventRecord(ctx->ev_pool[slot].b, ctx->stream);
    }
    StageTimer(const StageTimer &) = delete;
    StageTimer &operator=(const StageTimer &) = delete;
};

// call after the stream has been synchronised
void harvest_profile(icpmi_ctx *ctx)
{
    if (ctx->opt.profile && ctx->tgt.nn_engine == ICPMI_SEARCH_MFMA_BF16 && ctx->tgt.nn_misc.p) {
        unsigned long long cnt[MiscBlock::kCounterBytes / sizeof(unsigned long long)] = {0, 0, 0};
        if (hipMemcpy(cnt, ctx->tgt.counters(), sizeof(cnt), hipMemcpyDeviceToHost) == hipSuccess) {
            ctx->prof.nn_recheck_queries += (int64_t)cnt[0];
            ctx->prof.nn_fallback_queries += (int64_t)cnt[1];
            ctx->prof.nn_pruned_blocks += (int64_t)cnt[2];
            (void)hipMemset(ctx->tgt.counters(), 0, sizeof(cnt));
        }
    }
    for (size_t i = 0; i < ctx->ev_used; ++i) {
        float ms = 0.f;
        EventPair &p = ctx->ev_pool[i];
        if (hipEventElapsedTime(&ms, p.a, p.b) != hipSuccess) continue;
        switch (p.stage) {
        case ST_NN: ctx->prof.nn_ms += ms; ctx->prof.nn_launches++; break;
        case ST_REDUCE: ctx->prof.reduce_ms += ms; ctx->prof.reduce_launches++; break;
        case ST_TRANSFORM: ctx->prof.transform_ms += ms; ctx->prof.transform_launches++; break;
        case ST_NORMALS: ctx->prof.normals_ms += ms; ctx->prof.normals_launches++; break;
        case ST_TOTAL: ctx->prof.total_ms += ms; ctx->prof.calls++; break;
        case ST_LOOP: ctx->prof.loop_ms += ms; break;
        case ST_SETUP: ctx->prof.setup_ms += ms; break;
        case ST_COARSE: ctx->prof.coarse_ms += ms; ctx->prof.coarse_launches++; break;
        case ST_EXCHANGE: ctx->prof.exchange_ms += ms; ctx->prof.exchange_launches++; break;
        default: break;
        }
    }
    ctx->ev_used = 0;
}

// ---- kernel launch wrappers ------------------------------------------------------------

// Smallest target for which AUTO takes the MFMA engine (and its k-NN path); both engines return the
// same answers.  Round 1 had 8192 here, chosen on the 1-NN pass alone; the exact k-NN kernel (one
// thread per row, serial over the targets) costs 2.3 us per target point, so a 7.4k-point frame spent
// 17.6 ms in normal estimation where the MFMA path takes 0.2 ms (1.5k points 4.15 -> 0.39 ms per
// registration, 8k points 17.7 -> 0.44 ms).
// The MFMA engine still wins at 300 points (1.5 vs 2.6 ms for 50 iterations, 0.2 vs 0.8 ms of
// normals); below 256 targets a split is mostly padding and the exact kernels are kept.
constexpr int kMfmaMinTargets = 256; // (and sources of at least kMfmaMinQueries rows: loop_plan.h)

// Single-GPU loop: final sum, step and pose update in one launch (k_finish_step_transform).
// ICPMI_FUSE_FINISH=0 keeps the two separate kernels (the A/B knob of scripts/ab_fuse_finish.sh).
bool fuse_finish_enabled()
{
    static const bool v = [] {
        const char *e = getenv("ICPMI_FUSE_FINISH");
        return !(e && e[0] == '0' && e[1] == '\0');
    }();
    return v;
}
// (workgroups of the fused kernel, each of which repeats the final sum: finish_transform_blocks, loop_plan.h)

// ICPMI_SMALL=0 switches the small-cloud kernel off (loop_plan.h, kSmallMaxQueries)
bool small_enabled()
{
    static const bool v = [] {
        const char *e = getenv("ICPMI_SMALL");
        return !(e && e[0] == '0' && e[1] == '\0');
    }();
    return v;
}
// ICPMI_SMALL_MAX_SPLITS moves its limit of splits (loop_plan.h, kSmallSplitsDefault)
int small_max_splits()
{
    static const int v = [] {
        if (const char *e = getenv("ICPMI_SMALL_MAX_SPLITS")) {
            const long x = strtol(e, nullptr, 10);
            if (x >= 0 && x <= kSmallMaxSplits) return (int)x;
        }
        return kSmallSplitsDefault;
    }();
    return v;
}
// what a call's form is decided from (loop_plan.h), first the part the prepared target alone gives
LoopFacts target_facts(const icpmi_ctx *ctx)
{
    LoopFacts f;
    f.nn_engine = ctx->tgt.nn_engine;
    f.nn_pruned = ctx->tgt.nn_pruned;
    f.nn_splits = ctx->tgt.nn_splits;
    f.sw_small = small_enabled();
    f.sw_small_max_splits = small_max_splits();
    return f;
}

// Choose and prepare the search engine for a target cloud (once per call: the target does
// not move).  Both engines return the same indices; AUTO takes the MFMA engine once the
// pair count makes its fixed costs (Morton sort, operand packing, resolve) worthwhile.
// AUTO: the exact fp64 kernels for tiny clouds; the MFMA engine from 256 targets -- over all pairs while the target is
// a dozen splits or fewer (the small-cloud kernel of icp_small.h up to 8, the general kernels to 12), culled
// (nn_culled.h) beyond: the same correspondences bit for bit, 90-98 % of the (row tile, split) pairs never evaluated (round 4).
// (targets of more than kAutoCulledFrom splits.  scripts/engine_threshold.py: at 10 splits the culled engine's own fixed
// costs -- the rows' Morton sort, the lists -- still lose to the all-pairs kernels by 5-7 %, at 14 it wins by 7-13 %, at 49
// by 2.3-3.1x)
constexpr int kAutoCulledFrom = 12;
int engine_for(const icpmi_ctx *ctx, int m, int n_hint)
{
    int engine = ctx->opt.search;
    const int splits = (m + kSplitTargets - 1) / kSplitTargets;
    if (engine == ICPMI_SEARCH_AUTO) {
        engine = (m >= kMfmaMinTargets && n_hint >= kMfmaMinQueries) ? ICPMI_SEARCH_MFMA_BF16 : ICPMI_SEARCH_EXACT_F64;
        if (engine == ICPMI_SEARCH_MFMA_BF16 && splits > kAutoCulledFrom) engine = ICPMI_SEARCH_MFMA_PRUNED;
    }
    // (the culled coarse kernel keeps running sums over the splits in LDS: beyond kCullMaxSplits -- 6.3M targets -- all pairs)
    // (and the length of a split's list in 20 bits: fewer than 2^20 tiles of 32 rows)
    if (engine == ICPMI_SEARCH_MFMA_PRUNED && (splits > kCullMaxSplits || n_hint >= kCullMaxRows)) engine = ICPMI_SEARCH_MFMA_BF16;
    return engine;
}

int prepare_nn(icpmi_ctx *ctx, const double *d_tgt, int m, int n_hint)
{
    ctx->tgt.prep_valid = false; // whatever target the buffers held: it is being replaced
    int engine = engine_for(ctx, m, n_hint);
    // the culled engine is the MFMA engine plus the box test of (row group, split) pairs in the ICP loop and in normal
    // estimation; the stand-alone 1-NN search (nearest_batch) runs over all pairs
    ctx->tgt.nn_pruned = engine == ICPMI_SEARCH_MFMA_PRUNED;
    if (ctx->tgt.nn_pruned) engine = ICPMI_SEARCH_MFMA_BF16;
    ctx->tgt.nn_engine = engine;
    if (engine != ICPMI_SEARCH_MFMA_BF16) return ICPMI_OK;
    if (m >= (1 << 27)) return fail(ctx, ICPMI_ERR_ARG, "the MFMA engines take targets of fewer than 2^27 points (32-bit byte offsets into the sorted records)");
    const int splits = (m + kSplitTargets - 1) / kSplitTargets;
    ctx->tgt.nn_splits = splits;
    ctx->tgt.m = m;
    int rc;
    const int bblocks = std::max(1, std::min(256, (m + 255) / 256));
    size_t sort_bytes = 0;
    HIP_TRY(ctx, sort_pairs_u32(nullptr, &sort_bytes, nullptr, nullptr, nullptr, nullptr, (unsigned)m, ctx->stream));
    if ((rc = reserve(ctx, ctx->tgt.bpack, sizeof(uint4) * kSplitTiles * 64 * (size_t)splits))) return rc;
    if ((rc = reserve(ctx, ctx->bbox_part, sizeof(double) * 6 * (size_t)bblocks))) return rc;
    if ((rc = reserve(ctx, ctx->tgt.nn_misc, MiscBlock::kBytes))) return rc;
    if ((rc = reserve(ctx, ctx->tgt.sort_keys, SortPlanes(nullptr, (size_t)m).bytes))) return rc;
    if ((rc = reserve(ctx, ctx->sort_tmp, sort_bytes))) return rc;
    const int ms = (m + 63) / 64 * 64; // component stride of the SoA sorted copy
    ctx->tgt.nn_ms = ms;
    if ((rc = reserve(ctx, ctx->tgt.tgt_sorted, sizeof(double) * sorted_doubles(ms)))) return rc; // three planes + the records (nn_mfma.h)
    if ((rc = reserve(ctx, ctx->tgt.frames, frames_bytes(splits)))) return rc; // split frames, then the slots' boxes
    NnFrame *frame = ctx->tgt.frame();
    const SortPlanes sp(ctx->tgt.sort_keys.p, (size_t)m);
    hipStream_t s = ctx->stream;
    Range range("icpmi:target_prepass");
    StageTimer t(ctx, ST_SETUP);
    unsigned long long *stat3 = ctx->tgt.counters(); // the resolve's statistics words of the coming call
    if (m <= kBboxSingleMax)
        hipLaunchKernelGGL(k_bbox_single, dim3(1), dim3(1024), 0, s, d_tgt, m, frame, 1, stat3);
    else {
        hipLaunchKernelGGL(k_bbox_partial, dim3(bblocks), dim3(256), 0, s, d_tgt, m, (double *)ctx->bbox_part.p, 1);
        hipLaunchKernelGGL(k_bbox_final, dim3(1), dim3(64), 0, s, (const double *)ctx->bbox_part.p, bblocks, frame);
        HIP_TRY(ctx, hipMemsetAsync(stat3, 0, MiscBlock::kCounterBytes, s));
    }
    hipLaunchKernelGGL(k_morton_keys, dim3((m + 255) / 256), dim3(256), 0, s, d_tgt, m, (const NnFrame *)frame,
                       sp.keys_in, sp.vals_in);
    HIP_TRY(ctx, sort_pairs_u32(ctx->sort_tmp.p, &sort_bytes, sp.keys_in, sp.keys_out, sp.vals_in, sp.perm, (unsigned)m, s));
    hipLaunchKernelGGL(k_gather_points_rec, dim3((m + 255) / 256), dim3(256), 0, s, d_tgt, (const unsigned *)sp.perm, m, ms,
                       (double *)ctx->tgt.tgt_sorted.p);
    hipLaunchKernelGGL(k_split_frames, dim3(splits), dim3(256), 0, s, ctx->tgt.sorted(), m, ms,
                       (SplitFrame *)ctx->tgt.frames.p);
    hipLaunchKernelGGL(k_pack_targets, dim3((splits * kSplitTiles * 64 + 255) / 256), dim3(256), 0, s,
                       ctx->tgt.sorted(), m, ms, ctx->tgt.split_frames(),
                       (uint4 *)ctx->tgt.bpack.p, splits);
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

// an on / off switch of the environment: on unless its value starts with 0
bool env_on(const char *name)
{
    const char *e = getenv(name);
    return !(e && e[0] == '0');
}

// ICPMI_NN_BOUNDED=0: every pass of the ICP loop keeps its coarse minima and certifies afterwards (round 2's form)
// (read at every call, so that one process can run both forms on the same input: scripts/fuzz_bounded.py)
bool nn_bounded_enabled() { return env_on("ICPMI_NN_BOUNDED"); }

// ICPMI_NN_REUSE=0: every bounded pass of the all-pairs engine lists every row again (the form before list reuse; read at
// every call like ICPMI_NN_BOUNDED).  The skin (a fraction of a row's sqrt(ub)) and the looseness limit: RowBounds.
bool nn_reuse_enabled() { return env_on("ICPMI_NN_REUSE"); }
constexpr double kNnSkin = 0.5, kNnLoose = 8.0; // (the sweep: DESIGN.md, "List reuse")

// ICPMI_NN_MARGIN=0: no row's match is certified by its margin (list_reuse.h, "the match margin"): the launches and bits of
// the form before it.  Read at every call like ICPMI_NN_REUSE; on only where list reuse is and the loop's resolve is
// k_nn_resolve_bounded (sources of more than 32,768 rows), ungated.
bool nn_margin_enabled() { return env_on("ICPMI_NN_MARGIN"); }

// Lean passes (list_reuse.h, "lean passes").  ICPMI_NN_LEAN=0: every pass launches k_row_list and the coarse
// kernel, the launches of the form before lean passes -- the reference leg of tests and A/B runs.  ICPMI_NN_LEAN_FROM=k
// (k >= 2) is a TEST HOOK: every pass from the k-th on is lean whatever the counts say, which is the only way to put many
// rows through a lean pass's exhaustive search.  Both are read at every call like ICPMI_NN_MARGIN.
bool nn_lean_enabled() { return env_on("ICPMI_NN_LEAN"); }
// Culled full passes (LoopPlan::cull_full, loop_plan.h).  ICPMI_NN_CULL_FULL=0: a call's first two passes
// evaluate all pairs, the launches of the form before -- the reference leg of tests and A/B runs.  Read at every call.
bool nn_cull_full_enabled() { return env_on("ICPMI_NN_CULL_FULL"); }
int nn_lean_from()
{
    const char *e = getenv("ICPMI_NN_LEAN_FROM");
    const int k = e ? atoi(e) : 0;
    return k >= 2 ? k : 0;
}
// Solo passes (solo_pass.h).  ICPMI_NN_SOLO=0: a settled pass is the three launches of the form before -- the
// reference leg of tests and A/B runs.  ICPMI_NN_SOLO_FROM=k (k >= 2) is a TEST HOOK: the tail of every pass from the k-th on
// is the solo kernel whatever the counts say, the only way to put many rows through its exhaustive search.  Both are read
// at every call like ICPMI_NN_LEAN.
bool nn_solo_enabled() { return env_on("ICPMI_NN_SOLO"); }
int nn_solo_from()
{
    const char *e = getenv("ICPMI_NN_SOLO_FROM");
    const int k = e ? atoi(e) : 0;
    return k >= 2 ? k : 0;
}

// (The per-row arrays of the bounded pass inside ctx->nn_lists, list reuse's words, packed list and statistics, the match
// margin's records: BoundedRows, workspace_layout.h.)

// The culled engine's group lists (nn_culled.h) inside ctx->grp_cnt / grp_items: the counters, statistics and chunk counters
// of GroupCounters (workspace_layout.h) and one array of lists.
GroupCounters group_counters(const icpmi_ctx *ctx) { return GroupCounters(ctx->grp_cnt.p, (size_t)ctx->tgt.nn_splits); }
int reserve_group_lists(icpmi_ctx *ctx, int splits, long groups)
{
    int rc;
    if ((rc = reserve(ctx, ctx->grp_cnt, GroupCounters(nullptr, (size_t)splits).bytes))) return rc;
    const long cap = GroupCounters::items_cap(groups);
    if ((rc = reserve(ctx, ctx->grp_items, GroupCounters::items_bytes((size_t)splits, cap)))) return rc;
    ctx->grp_cap = (int)cap;
    return ICPMI_OK;
}
GroupLists group_lists(const icpmi_ctx *ctx, int set) { return GroupLists{group_counters(ctx).set[set], (unsigned *)ctx->grp_items.p, ctx->grp_cap}; }
// workgroups of k_nn_coarse_groups (kCoarseWaves pairs each): the chip's resident set, two per CU at 4 waves per SIMD; a
// workgroup starts on chunk blockIdx and takes its next ones from a counter (nn_culled.h)
int coarse_groups_grid(const icpmi_ctx *ctx) { return 2 * ctx->cu_count; }
size_t coarse_groups_lds(int splits) { return sizeof(unsigned) * (2 * (size_t)splits + 1); }

// One search of the ICP loop, as the loop's plan describes it; default-constructed: a stand-alone search over all pairs.
struct NnPass {
    int pruned_pass = -1; // the culled engine: which pass of the call (selects the set of group lists); -1: all-pairs engine
    bool bounded = false; // d_idx holds the rows' matches of the previous pass and the kernel that moved the rows has left
                          // their bounds in ctx->nn_lists (RowBounds, kernels.h; nn_bounded.h)
    bool list = false;    // list reuse: the coarse pass runs over the packed list of the rows listed again
    bool lean = false;    // a lean pass: no coarse launch
    bool margin = false;  // the match margin's resolve
    int culled_full = -1; // all-pairs engine, a culled full pass (LoopPlan::cull_full): which pass of the call, 0 or 1 (selects
                          // the set of group lists like pruned_pass); -1: not one
};
int launch_nn_mfma(icpmi_ctx *ctx, const double *d_qry, int n, int m, int *d_idx, double *d_d2,
                   const IcpState *st, const double *d_tgt = nullptr, const double *d_nrm = nullptr,
                   double *d_partials = nullptr, const NnPass &pass = NnPass{})
{
    const int splits = ctx->tgt.nn_splits;
    int rc;
    const SplitFrame *frames = ctx->tgt.split_frames();
    const unsigned *perm = ctx->tgt.perm();
    unsigned long long *counters = ctx->tgt.counters();
    Range range("icpmi:nn_search");
    StageTimer t(ctx, ST_NN);
    if (pass.bounded) {
        const BoundedRows lr(ctx->nn_lists.p, (size_t)n);
        // (a lean pass of the all-pairs engine -- list_reuse.h, "lean passes" -- has no coarse launch: the rows' kept lists and
        // certificates stand, and a row that wanted a new list takes the resolve's exhaustive search)
        if (!pass.lean) {
            StageTimer tc(ctx, ST_COARSE);
            const KnnLists kl{lr.ubf, lr.sqf, lr.cnt, lr.ent, kNnEntCap};
            if (pass.pruned_pass >= 0 || pass.culled_full >= 0) {
                // the culled engine's surviving (row group, split) pairs, list epilogue: a row's list then holds slots of
                // evaluated splits only, and every split that can hold a target within the row's bound IS evaluated (the
                // group's bound is the largest of its rows'); pass p reads the lists counted in set p & 1 and clears the other
                // (the all-pairs engine's culled full passes: the same launch on the same sets, nothing counted -- the pair
                // counters are the culled engine's)
                const bool full = pass.pruned_pass < 0;
                const int parity = (full ? pass.culled_full : pass.pruned_pass) & 1;
                const GroupLists cur = group_lists(ctx, parity), nxt = group_lists(ctx, parity ^ 1);
                const GroupCounters gc = group_counters(ctx);
                const long groups = (n + kGroupRows - 1) / kGroupRows;
                if (full) ctx->prof.nn_full_culled_passes += 1;
                hipLaunchKernelGGL((k_nn_coarse_groups<false, kCoarseWaves>), dim3(coarse_groups_grid(ctx)), dim3(kCoarseThreads),
                                   coarse_groups_lds(splits), ctx->stream, d_qry, n, (size_t)0, ctx->tgt.operands(), frames, splits,
                                   (const unsigned *)cur.items, cur.cap, (const unsigned *)cur.cnt, nxt.cnt,
                                   ctx->opt.profile && !full ? gc.stats : (unsigned long long *)nullptr, (unsigned long long)(groups * splits),
                                   st, kl, gc.work[parity], gc.work[parity ^ 1]);
            } else {
                // list reuse (`pass.list`): the pass runs over the packed list of the rows listed again (k_row_list) and no others
                const int *list = pass.list ? lr.list : nullptr;
                if (coarse_half_units(ctx->cu_count, n, splits)) {
                    constexpr int per = kCoarseQueries / kCoarseQT; // queries per workgroup with one tile per wave
                    hipLaunchKernelGGL((k_nn_coarse_bounded<1, kCoarseWaves>), dim3((n + per - 1) / per, splits), dim3(kCoarseThreads), 0,
                                       ctx->stream, d_qry, n, ctx->tgt.operands(), frames, kl, st, list);
                } else
                    hipLaunchKernelGGL((k_nn_coarse_bounded<kCoarseQT, kCoarseWaves>), dim3((n + kCoarseQueries - 1) / kCoarseQueries, splits),
                                       dim3(kCoarseThreads), 0, ctx->stream, d_qry, n, ctx->tgt.operands(), frames, kl, st, list);
            }
            ctx->prof.nn_coarse_blocks += (int64_t)((n + kCoarseQueries - 1) / kCoarseQueries) * splits;
        }
        // (the statistics: with one row in a hundred listing a second slot, most waves of a pass have something to add to the
        // same two words, and per wave those atomics were 25 of the kernel's 55 us -- they leave per workgroup now, and
        // only when the stage profile (level 2) is asked for)
#define ICPMI_BOUNDED_ARGS                                                                                                        \
    d_qry, n, ctx->tgt.sorted(), perm, m, ctx->tgt.nn_ms, splits, frames, (const double *)lr.ub, (const int *)lr.cnt, \
        (const unsigned *)lr.ent, d_idx, ctx->opt.profile >= 2 ? counters : (unsigned long long *)nullptr, d_tgt, d_nrm, d_partials, st
        if (resolve_waves(n) == 8)
            hipLaunchKernelGGL(k_nn_resolve4_bounded<8>, dim3(resolve_blocks(n)), dim3(512), 0, ctx->stream, ICPMI_BOUNDED_ARGS);
        else if (pass.margin) // (the match margin: certified rows are not scanned, scanned rows leave their new margin)
            hipLaunchKernelGGL(k_nn_resolve_bounded<true>, dim3(resolve_blocks(n)), dim3(64 * kResolveWW), 0, ctx->stream, ICPMI_BOUNDED_ARGS,
                               (const unsigned long long *)lr.cert, (const double *)lr.cover, lr.scan);
        else
            hipLaunchKernelGGL(k_nn_resolve_bounded<false>, dim3(resolve_blocks(n)), dim3(64 * kResolveWW), 0, ctx->stream, ICPMI_BOUNDED_ARGS,
                               (const unsigned long long *)nullptr, (const double *)nullptr, (RowScan *)nullptr);
#undef ICPMI_BOUNDED_ARGS
        if (!pass.list) ctx->prof.nn_pairs += (double)n * (double)m; // (a pass with list reuse: its workgroup columns that ran,
                                                                      // from the rows listed -- profiling only -- and added after the call)
        ctx->prof.bounded_launches += 1;
        HIP_TRY(ctx, hipGetLastError());
        return ICPMI_OK;
    }
    if (pass.pruned_pass >= 0) return fail(ctx, ICPMI_ERR_ARG, "internal: the culled engine has bounded passes only");
    if ((rc = reserve(ctx, ctx->coarse, coarse_bytes(splits, n)))) return rc;
    {
        StageTimer tc(ctx, ST_COARSE); // the dominant kernel alone (matches rocprofv3's per-kernel average)
        if (coarse_half_units(ctx->cu_count, n, splits)) {
            constexpr int per = kCoarseQueries / kCoarseQT; // queries per workgroup with one tile per wave
            hipLaunchKernelGGL((k_nn_coarse<0, 1, kCoarseWaves>), dim3((n + per - 1) / per, splits), dim3(kCoarseThreads), 0,
                               ctx->stream, d_qry, n, ctx->tgt.operands(), frames, (float2 *)ctx->coarse.p,
                               (float *)nullptr, st);
        } else {
            hipLaunchKernelGGL((k_nn_coarse<0, kCoarseQT, kCoarseWaves>), dim3((n + kCoarseQueries - 1) / kCoarseQueries, splits),
                               dim3(kCoarseThreads), 0, ctx->stream, d_qry, n, ctx->tgt.operands(), frames,
                               (float2 *)ctx->coarse.p, (float *)nullptr, st);
        }
        ctx->prof.nn_coarse_blocks += (int64_t)((n + kCoarseQueries - 1) / kCoarseQueries) * splits;
    }
    // (the two null lists: round 3's per-block split lists -- the culled engine no longer has unbounded passes)
#define ICPMI_RESOLVE_ARGS                                                                                            \
    d_qry, n, ctx->tgt.sorted(), perm, m, ctx->tgt.nn_ms, (const float2 *)ctx->coarse.p, splits, frames,  \
        ctx->tgt.frame(), d_idx, d_d2, counters, d_tgt, d_nrm, d_partials, (const int *)nullptr, (const int *)nullptr, st
    if (resolve_waves(n) == 8)
        hipLaunchKernelGGL(k_nn_resolve4<8>, dim3(resolve_blocks(n)), dim3(512), 0, ctx->stream, ICPMI_RESOLVE_ARGS);
    else
        hipLaunchKernelGGL(k_nn_resolve<16>, dim3(resolve_blocks(n)), dim3(64 * kResolveWW), 0, ctx->stream, ICPMI_RESOLVE_ARGS);
#undef ICPMI_RESOLVE_ARGS
    ctx->prof.nn_pairs += (double)n * (double)m;
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

// nearest neighbour of every row of d_qry among d_tgt -> d_idx (+ optional d_d2)
int launch_nn(icpmi_ctx *ctx, const double *d_qry, int n, const double *d_tgt, int m, int *d_idx,
              double *d_d2, const IcpState *st)
{
    if (ctx->tgt.nn_engine == ICPMI_SEARCH_MFMA_BF16) return launch_nn_mfma(ctx, d_qry, n, m, d_idx, d_d2, st);
    constexpr int QPT = 2;
    const int qblocks = (n + 256 * QPT - 1) / (256 * QPT);
    // enough workgroups to fill 256 CUs several times over; every split keeps >= 256 targets
    int splits = (8 * ctx->cu_count + qblocks - 1) / qblocks;
    splits = std::max(1, std::min(splits, std::min(64, (m + 255) / 256)));
    const int per = (m + splits - 1) / splits;
    splits = (m + per - 1) / per;
    int rc;
    if ((rc = reserve(ctx, ctx->part_d2, sizeof(double) * (size_t)splits * n))) return rc;
    if ((rc = reserve(ctx, ctx->part_idx, sizeof(int) * (size_t)splits * n))) return rc;
    Range range("icpmi:nn_search");
    StageTimer t(ctx, ST_NN);
    hipLaunchKernelGGL(k_nn_f64<QPT>, dim3(qblocks, splits), dim3(256), 0, ctx->stream, d_qry, n,
                       d_tgt, m, per, (double *)ctx->part_d2.p, (int *)ctx->part_idx.p, st);
    hipLaunchKernelGGL(k_nn_merge, dim3((n + 255) / 256), dim3(256), 0, ctx->stream,
                       (const double *)ctx->part_d2.p, (const int *)ctx->part_idx.p, n, splits,
                       d_idx, d_d2, st);
    ctx->prof.nn_pairs += (double)n * (double)m;
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

// Normal estimation takes the target's rows in Morton order (a rank's slice is then a range of sorted positions) with
// the pruned engine, whose blocks must be compact, and with the all-pairs engine's list form (knn_lists.h;
// ICPMI_KNN_LISTS=0: round 2's slot-minimum form, rows in point order)
bool knn_lists_enabled()
{
    static const bool on = env_on("ICPMI_KNN_LISTS");
    return on;
}
// The target's k-NN setup on the all-pairs engine culls its coarse pass like the culled engine's does (k_knn_group_cull +
// k_nn_coarse_groups<true>, nn_culled.h: they read the sorted target, the rows' bounds and the split boxes, which
// prepare_nn builds for both engines) once the target has more than kKnnCullFromSplits splits -- the size from which AUTO
// takes the culled engine (kAutoCulledFrom, profiles/r4_final/engine_threshold.json); at a dozen splits or fewer the
// all-pairs form stays, launch for launch.  ICPMI_KNN_CULL=0: the all-pairs coarse pass at every size (the reference leg of
// tests/test_gpu_knn_cull_allpairs.py).  The engine's ICP loop culls its first two passes over the same window of sizes
// (LoopPlan::cull_full, loop_plan.h, where the two limits live) and is all pairs from the third pass on.
static_assert(kKnnCullFromSplits == kAutoCulledFrom, "the all-pairs engine culls from the size AUTO takes the culled engine from");
bool knn_cull_enabled()
{
    static const bool on = env_on("ICPMI_KNN_CULL");
    return on;
}
bool knn_culled(const icpmi_ctx *ctx)
{
    return ctx->tgt.nn_pruned || (knn_cull_enabled() && ctx->tgt.nn_splits > kKnnCullFromSplits && ctx->tgt.nn_splits <= kCullMaxSplits);
}
bool sorted_normal_rows(const icpmi_ctx *ctx, int k, int m)
{
    return ctx->tgt.nn_engine == ICPMI_SEARCH_MFMA_BF16 && (ctx->tgt.nn_pruned || knn_lists_enabled()) && k <= 32 && m >= kMfmaMinTargets;
}

// k-NN lists of rows [row0,row1) of d_qry among the m points d_pts (kdtree.hpp:65-78): MFMA
// coarse pass + exact resolve, or the exact fp64 kernel.  List of row i -> ctx->knn_idx[i * k ..],
// closest first.  prepare_nn() must have run for d_pts.  d_qry == d_pts for normal estimation.
// With the pruned engine (`by_sorted_row`, d_qry == d_pts only), [row0, row1) are positions in the
// Morton-sorted target (row0 a multiple of 64).
int launch_knn(icpmi_ctx *ctx, const double *d_qry, int nq_total, const double *d_pts, int m, int k, int row0, int row1,
               bool by_sorted_row = false)
{
    const int rows = row1 - row0;
    if (rows <= 0) return ICPMI_OK;
    int rc;
    if ((rc = reserve(ctx, ctx->knn_idx, sizeof(int) * (size_t)std::max(m, nq_total) * k))) return rc;
    int *knn = (int *)ctx->knn_idx.p;
    hipStream_t s = ctx->stream;
    constexpr int BLOCK = 128;
    const size_t smem = (size_t)k * BLOCK * (sizeof(double) + sizeof(int));
    const bool mfma = ctx->tgt.nn_engine == ICPMI_SEARCH_MFMA_BF16 && k <= 32 && m >= kMfmaMinTargets;
    const unsigned *perm = mfma ? ctx->tgt.perm() : nullptr;
    const double *qsep = d_qry == d_pts ? nullptr : d_qry; // the exact kernels read rows from d_pts unless told otherwise
    if (by_sorted_row && (!mfma || qsep)) return fail(ctx, ICPMI_ERR_ARG, "sorted-row lists need the MFMA engine's sorted target");
    if (mfma) {
        const int splits = ctx->tgt.nn_splits, nslots = splits * kCols;
        // bound the per-row buffer (the lists, or 2 B x nslots of slot minima) by chunking the rows: ~1 GiB
        // all-pairs engine, rows in the target's Morton order: bound first, lists instead of minima (knn_lists.h)
        // (culled -- the pruned engine, and the all-pairs engine on targets of more than a dozen splits, knn_culled(): the same
        // lists on the units that survive the box test against the group's largest row bound)
        const bool lists = by_sorted_row; // (round 3's block lists over slot minima for the culled engine are gone)
        const bool lists_culled = lists && knn_culled(ctx);
        // rows that are not a range of sorted positions (arbitrary queries: icpmi_k_nearest; rows by point index:
        // icpmi_estimate_normals_rows) get their place in the sorted order from their Morton key (k_knn_prebound_q)
        const bool lists_q = !by_sorted_row && knn_lists_enabled();
        constexpr long budget = 1l << 30;
        long chunk = (budget / ((lists || lists_q) ? (long)KnnRows::kRowBytes : (long)nslots * 2)) / kCoarseQueries * kCoarseQueries; // 2 bytes per slot minimum (bf16)
        chunk = std::max<long>(kCoarseQueries, std::min<long>(chunk, ((long)rows + kCoarseQueries - 1) / kCoarseQueries * kCoarseQueries));
        if ((rc = reserve(ctx, ctx->slotmin, (lists || lists_q) ? KnnRows(nullptr, (size_t)chunk).bytes : sizeof(unsigned short) * (size_t)chunk * nslots))) return rc;
        if ((rc = reserve(ctx, ctx->fb_list, sizeof(int) * ((size_t)rows + 16)))) return rc;
        int *fb_count = (int *)ctx->fb_list.p, *fb_list = fb_count + 16;
        // (the list forms: a chunk's first kernel, k_knn_prebound / k_knn_prebound_q, clears fb_count before the first chunk
        // and the group counters before every chunk -- knn_lists.h)
        if (!lists && !lists_q) HIP_TRY(ctx, hipMemsetAsync(fb_count, 0, sizeof(int), s));
        const SplitFrame *frames = ctx->tgt.split_frames();
        const double *sorted = ctx->tgt.sorted();
        if (lists_culled && (rc = reserve_group_lists(ctx, splits, chunk / kGroupRows))) return rc;
        // (the list forms' rows of a chunk, and the group counters the culled one clears and counts in)
        const KnnRows kr(ctx->slotmin.p, (size_t)chunk);
        const KnnLists kl{kr.tf_row, kr.sqf_row, kr.cnt_row, kr.ent_row, kKnnEntCap};
        const GroupCounters gc = group_counters(ctx);
        for (long c0 = row0; c0 < row1; c0 += chunk) {
            const int nq = (int)std::min<long>(chunk, row1 - c0);
            const int nblk = (nq + kCoarseQueries - 1) / kCoarseQueries;
            if (lists) {
                hipLaunchKernelGGL(k_knn_prebound, dim3((nq + kPreRows - 1) / kPreRows), dim3(256), 0, s, sorted, m, ctx->tgt.nn_ms, k, (int)c0, nq,
                                   kr.t_row, kr.tf_row, kr.sqf_row, kr.cnt_row, c0 == row0 ? fb_count : (int *)nullptr,
                                   lists_culled ? (unsigned *)ctx->grp_cnt.p : (unsigned *)nullptr,
                                   lists_culled ? (int)(gc.bytes / sizeof(unsigned)) : 0);
                if (lists_culled) {
                    // the groups are runs of 32 sorted rows, their bound the largest of their rows' (nn_culled.h); a wave takes two
                    const GroupLists gl = group_lists(ctx, 0);
                    const int waves = (nq + 63) / 64;
                    ctx->prof.knn_culled_launches += 1;
                    hipLaunchKernelGGL(k_knn_group_cull, dim3((waves + 15) / 16), dim3(1024), 0, s, sorted, m, ctx->tgt.nn_ms, (int)c0, nq,
                                       (const double *)kr.t_row, frames, splits, gl);
                    hipLaunchKernelGGL((k_nn_coarse_groups<true, kCoarseWaves>), dim3(coarse_groups_grid(ctx)), dim3(kCoarseThreads),
                                       coarse_groups_lds(splits), s, sorted + c0, nq, (size_t)ctx->tgt.nn_ms, ctx->tgt.operands(), frames,
                                       splits, (const unsigned *)gl.items, gl.cap, (const unsigned *)gl.cnt, (unsigned *)nullptr,
                                       (unsigned long long *)nullptr, 0ull, (const IcpState *)nullptr, kl, gc.work[0],
                                       (unsigned *)nullptr);
                } else if (coarse_half_units(ctx->cu_count, nq, splits)) {
                    constexpr int per = kCoarseQueries / kCoarseQT;
                    hipLaunchKernelGGL((k_nn_coarse_rows<1, kCoarseWaves>), dim3((nq + per - 1) / per, splits), dim3(kCoarseThreads), 0,
                                       s, sorted + c0, nq, (size_t)ctx->tgt.nn_ms, ctx->tgt.operands(), frames, kl);
                } else
                    hipLaunchKernelGGL((k_nn_coarse_rows<kCoarseQT, kCoarseWaves>), dim3(nblk, splits), dim3(kCoarseThreads), 0, s,
                                       sorted + c0, nq, (size_t)ctx->tgt.nn_ms, ctx->tgt.operands(), frames, kl);
                hipLaunchKernelGGL(k_knn_resolve_lists<false>, dim3((nq + 3) / 4), dim3(256), 0, s, (const double *)nullptr, sorted, perm, m,
                                   ctx->tgt.nn_ms, k, (int)c0, nq, (const double *)kr.t_row, (const int *)kr.cnt_row, (const unsigned *)kr.ent_row, knn,
                                   fb_list, fb_count);
            } else if (lists_q) {
                hipLaunchKernelGGL(k_knn_prebound_q, dim3((nq + 7) / 8), dim3(256), 0, s, d_qry, (int)c0, nq, sorted,
                                   ctx->tgt.sorted_keys(), m, ctx->tgt.nn_ms, k,
                                   ctx->tgt.frame(), kr.t_row, kr.tf_row, kr.sqf_row, kr.cnt_row,
                                   c0 == row0 ? fb_count : (int *)nullptr);
                if (coarse_half_units(ctx->cu_count, nq, splits)) {
                    constexpr int per = kCoarseQueries / kCoarseQT;
                    hipLaunchKernelGGL((k_nn_coarse_bounded<1, kCoarseWaves>), dim3((nq + per - 1) / per, splits), dim3(kCoarseThreads), 0,
                                       s, d_qry + 3 * c0, nq, ctx->tgt.operands(), frames, kl, (const IcpState *)nullptr);
                } else
                    hipLaunchKernelGGL((k_nn_coarse_bounded<kCoarseQT, kCoarseWaves>), dim3(nblk, splits), dim3(kCoarseThreads), 0, s,
                                       d_qry + 3 * c0, nq, ctx->tgt.operands(), frames, kl, (const IcpState *)nullptr);
                hipLaunchKernelGGL(k_knn_resolve_lists<true>, dim3((nq + 3) / 4), dim3(256), 0, s, d_qry, sorted, perm, m, ctx->tgt.nn_ms, k,
                                   (int)c0, nq, (const double *)kr.t_row, (const int *)kr.cnt_row, (const unsigned *)kr.ent_row, knn, fb_list,
                                   fb_count);
            } else {
                if (coarse_half_units(ctx->cu_count, nq, splits)) {
                    constexpr int per = kCoarseQueries / kCoarseQT;
                    hipLaunchKernelGGL((k_nn_coarse<1, 1, kCoarseWaves>), dim3((nq + per - 1) / per, splits),
                                       dim3(kCoarseThreads), 0, s, d_qry + 3 * c0, nq, ctx->tgt.operands(),
                                       frames, (float2 *)nullptr, (float *)ctx->slotmin.p, (const IcpState *)nullptr);
                } else
                hipLaunchKernelGGL((k_nn_coarse<1, kCoarseQT, kCoarseWaves>), dim3(nblk, splits),
                                   dim3(kCoarseThreads), 0, s, d_qry + 3 * c0, nq, ctx->tgt.operands(),
                                   frames, (float2 *)nullptr, (float *)ctx->slotmin.p, (const IcpState *)nullptr);
                hipLaunchKernelGGL(k_knn_resolve<false>, dim3((nq + 3) / 4), dim3(256), 0, s, d_qry, (int)c0, nq, sorted, perm, m,
                                   ctx->tgt.nn_ms, k, (const float *)ctx->slotmin.p, nslots, frames, ctx->tgt.frame(), knn,
                                   fb_list, fb_count, (const int *)nullptr, (const int *)nullptr);
            }
        }
        hipLaunchKernelGGL(k_knn_exact_rows, dim3((lists || lists_q) ? ctx->cu_count : 1024), dim3(256), (size_t)k * 256 * (sizeof(double) + sizeof(int)),
                           s, d_pts, m, k, (const int *)fb_list, (const int *)fb_count, knn,
                           by_sorted_row ? perm : (const unsigned *)nullptr, qsep);
        if (ctx->opt.profile) { // visibility only: how many rows took the exact path
            int cnt = 0;
            HIP_TRY(ctx, hipMemcpyAsync(&cnt, fb_count, sizeof(int), hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
            ctx->prof.knn_fallback_rows += cnt;
        }
    } else {
        hipLaunchKernelGGL(k_knn_exact_list<BLOCK>, dim3((rows + BLOCK - 1) / BLOCK), dim3(BLOCK), smem, s,
                           d_pts, m, k, row0, row1, (const int *)nullptr, (const int *)nullptr, knn, qsep);
    }
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

// normals of rows [row0,row1) of d_pts against all m points (icp.hpp:23-67): k-NN lists then PCA.
// With the pruned engine (`by_sorted_row`) the rows are sorted positions and `scatter` selects
// where a normal goes: to its point's row of d_normals (m rows), or to its sorted row (what a
// rank contributes to the all-gather).
int launch_normals(icpmi_ctx *ctx, const double *d_pts, int m, int k, int row0, int row1,
                   double *d_normals, bool by_sorted_row = false, bool scatter = true)
{
    const int rows = row1 - row0;
    if (rows <= 0) return ICPMI_OK;
    int rc;
    Range range("icpmi:normals");
    StageTimer t(ctx, ST_NORMALS);
    if ((rc = launch_knn(ctx, d_pts, m, d_pts, m, k, row0, row1, by_sorted_row))) return rc;
    const bool mfma = ctx->tgt.nn_engine == ICPMI_SEARCH_MFMA_BF16 && k <= 32 && m >= kMfmaMinTargets;
    const unsigned *perm = mfma ? ctx->tgt.perm() : nullptr;
    hipLaunchKernelGGL(k_normals_from_knn, dim3((rows + 255) / 256), dim3(256), 0, ctx->stream, d_pts, m, k, row0, row1,
                       (const int *)ctx->knn_idx.p, d_normals, by_sorted_row ? perm : (const unsigned *)nullptr,
                       (int)(by_sorted_row && scatter));
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

int check_common(icpmi_ctx *ctx)
{
    if (!ctx) return ICPMI_ERR_NULL;
    HIP_TRY(ctx, hipSetDevice(ctx->opt.device));
    if (ctx->trailing_work) {
        // The previous icpmi_stream_push* returned with the preparation of its NEXT target (Morton sort, operand
        // packing, 20-NN, normals) still queued.  A fault in those kernels belongs to that step, not to whatever
        // this call is about to do: look before queueing anything behind it.
        ctx->trailing_work = false;
        const hipError_t e = hipStreamQuery(ctx->stream);
        if (e != hipSuccess && e != hipErrorNotReady) {
            (void)hipGetLastError();
            ctx->tgt.prep_valid = false;
            return fail(ctx, ICPMI_ERR_HIP, "the target preparation queued behind the previous icpmi_stream_push failed: %s",
                        hipGetErrorString(e));
        }
    }
    return ICPMI_OK;
}

int load_rccl(icpmi_ctx *ctx)
{
    Rccl &r = ctx->rccl;
    if (r.lib) return ICPMI_OK;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *nm : names) {
        r.lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
        if (r.lib) break;
    }
    if (!r.lib) return fail(ctx, ICPMI_ERR_RCCL, "cannot dlopen librccl: %s", dlerror());
#define SYM(field, name)                                                                      \
    r.field = reinterpret_cast<decltype(r.field)>(dlsym(r.lib, name));                        \
    if (!r.field) return fail(ctx, ICPMI_ERR_RCCL, "librccl lacks %s", name)
    SYM(GetUniqueId, "ncclGetUniqueId");
    SYM(CommInitRank, "ncclCommInitRank");
    SYM(CommDestroy, "ncclCommDestroy");
    SYM(AllReduce, "ncclAllReduce");
    SYM(AllGather, "ncclAllGather");
    SYM(GetErrorString, "ncclGetErrorString");
    SYM(CommCount, "ncclCommCount");
    SYM(CommUserRank, "ncclCommUserRank");
    SYM(CommCuDevice, "ncclCommCuDevice");
#undef SYM
    return ICPMI_OK;
}

#define RCCL_TRY(ctx, expr)                                                                   \
    do {                                                                                      \
        ncclResult_t r_ = (expr);                                                             \
        if (r_ != ncclSuccess)                                                                \
            return fail(ctx, ICPMI_ERR_RCCL, "%s failed: %s", #expr,                          \
                        ctx->rccl.GetErrorString(r_));                                        \
    } while (0)

// ---- exchanges of the sharded path --------------------------------------------------------
// in-place sum of `count` doubles at device address d_buf over all ranks
int exchange_allreduce(icpmi_ctx *ctx, double *d_buf, int count)
{
    if (ctx->comm) {
        RCCL_TRY(ctx, ctx->rccl.AllReduce(d_buf, d_buf, count, ncclDouble, ncclSum, ctx->comm, ctx->stream));
        return ICPMI_OK;
    }
    ctx->cb_host.resize(std::max<size_t>(ctx->cb_host.size(), count));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->cb_host.data(), d_buf, sizeof(double) * count, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->cb_allreduce(ctx->cb_user, ctx->cb_host.data(), count) != 0)
        return fail(ctx, ICPMI_ERR_RCCL, "all-reduce callback failed");
    HIP_TRY(ctx, hipMemcpyAsync(d_buf, ctx->cb_host.data(), sizeof(double) * count, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ICPMI_OK;
}

// in-place all-gather: rank r's `per` doubles sit at d_buf + r * per
int exchange_allgather(icpmi_ctx *ctx, double *d_buf, size_t per)
{
    if (ctx->comm) {
        RCCL_TRY(ctx, ctx->rccl.AllGather(d_buf + (size_t)ctx->rank * per, d_buf, per, ncclDouble, ctx->comm, ctx->stream));
        return ICPMI_OK;
    }
    const size_t total = per * ctx->n_ranks;
    ctx->cb_host.resize(std::max(ctx->cb_host.size(), total));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->cb_host.data(), d_buf, sizeof(double) * total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->cb_allgather(ctx->cb_user, ctx->cb_host.data(), (int32_t)per) != 0)
        return fail(ctx, ICPMI_ERR_RCCL, "all-gather callback failed");
    HIP_TRY(ctx, hipMemcpyAsync(d_buf, ctx->cb_host.data(), sizeof(double) * total, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ICPMI_OK;
}

// The target normals (ctx->tgt.nrm, by point) once more in the target's Morton order, for the small-cloud
// kernel: its slot scans then read a candidate's normal next to its coordinates.
int sort_normals(icpmi_ctx *ctx, int m)
{
    if (!small_target(target_facts(ctx))) return ICPMI_OK;
    int rc;
    if ((rc = reserve(ctx, ctx->tgt.nrm_sorted, sizeof(double) * 3 * (size_t)ctx->tgt.nn_ms))) return rc;
    hipLaunchKernelGGL(k_gather_points, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, (const double *)ctx->tgt.nrm.p,
                       ctx->tgt.perm(), m, ctx->tgt.nn_ms, (double *)ctx->tgt.nrm_sorted.p);
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

// A target prepared on a helper context (prepare_target on its stream and workspace) becomes this context's:
// what DEFINES a prepared target (PreparedTarget) changes hands (the helper gets this context's old one to build the
// next target in), scratch stays where it is.  The caller orders this context's stream behind the helper's work.
void adopt_target(icpmi_ctx *ctx, icpmi_ctx *h)
{
    std::swap(ctx->tgt, h->tgt); // (the helper reads none of the scalars it is handed before its next prepare_nn rewrites them)
    ctx->tgt.prep_valid = true;
    h->tgt.prep_valid = false;
}

// ---- the ICP call, device pointers -----------------------------------------------------
// Search structure + normals of a target for a single-GPU registration (icp.hpp:169-171), queued on the
// context's stream; remembered, so that an align against the same device pointer and size with the
// same engine finds them in place.  Everything else that prepares a search (prepare_nn) forgets it.
int prepare_target(icpmi_ctx *ctx, const double *d_tgt, int m, int n_hint)
{
    int rc;
    if ((rc = reserve(ctx, ctx->tgt.nrm, sizeof(double) * 3 * (size_t)m))) return rc;
    if ((rc = prepare_nn(ctx, d_tgt, m, n_hint))) return rc;
    const bool sorted_rows = sorted_normal_rows(ctx, ctx->opt.normal_k, m);
    if ((rc = launch_normals(ctx, d_tgt, m, ctx->opt.normal_k, 0, m, (double *)ctx->tgt.nrm.p, sorted_rows, true))) return rc;
    if ((rc = sort_normals(ctx, m))) return rc;
    ctx->tgt.prep_tgt = d_tgt;
    ctx->tgt.prep_m = m;
    ctx->tgt.prep_engine = engine_for(ctx, m, n_hint);
    ctx->tgt.prep_valid = true;
    return ICPMI_OK;
}

// The correspondence-distance gate of a registration (icp_gated.h): null means none, and every branch below is then
// what it was before the gate existed.
// With a kind it is a robust rule as well (icp_robust.h): the rows that pass g2 (DBL_MAX: no gate) are weighted, the
// robust kernels run in the gated ones' places, the weight sum is the state's sums[28] and the pairs its sums[29].
// Without a kind the gated kernels run, unchanged.
struct GateRun {
    double g2;     // max_distance * max_distance
    int64_t pairs; // out: the rows kept by the pass that produced final_error (the state's sums[28], which comes back anyway)
    int32_t kind = 0;        // ICPMI_ROBUST_* (0: the gate alone)
    double ks = 0.0;         // the kernels' scale: k for Huber, k * k for Geman-McClure
    double weight_sum = 0.0; // out: the weight sum of that same pass
    // Plane-to-plane rows (icp_gicp.h): k_reduce_gicp runs in k_reduce_gated's place at every size, behind g2 (DBL_MAX: no
    // gate), over the source's normals that align_device estimates first; the step kernel and the outputs are the gate's.
    bool gicp = false;
    double c = 0.0, kappa = 0.0; // 1 - epsilon, 2 * epsilon
    // ICPMI_GICP_FORM_SMALL: at the small-cloud kernel's sizes (LoopFacts::gicp_small) the passes run k_icp_small_gicp
    bool gicp_small = false;
};
static_assert(kRobustHuber == ICPMI_ROBUST_HUBER && kRobustGemanMcClure == ICPMI_ROBUST_GEMAN_MCCLURE, "the kernels' kinds are the header's");

LoopRule rule_of(const GateRun *gate) { return !gate ? kRuleNone : gate->gicp ? kRuleGicp : gate->kind ? kRuleRobust : kRuleGate; }

// One launch of the kernel that the call's rule selects out of a plain / gated / robust triple whose arguments differ only in
// the rule's own, which go behind the common ones (k_reduce*, k_icp_small*).
template <class... PA, class... GA, class... RA, class... A>
void launch_by_rule(const GateRun *gate, void (*plain)(PA...), void (*gated)(GA...), void (*robust)(RA...), dim3 grid, dim3 block,
                    hipStream_t s, A... common)
{
    switch (rule_of(gate)) {
    case kRuleRobust: hipLaunchKernelGGL(robust, grid, block, 0, s, common..., gate->g2, (int)gate->kind, gate->ks); break;
    case kRuleGate: hipLaunchKernelGGL(gated, grid, block, 0, s, common..., gate->g2); break;
    case kRuleNone: hipLaunchKernelGGL(plain, grid, block, 0, s, common...); break;
    // (no member of these triples: LoopRun::pass_sums launches k_reduce_gicp and LoopRun::queue_pass_small k_icp_small_gicp
    // themselves, and make_loop_plan refuses -- LoopPlan::error, the call fails in settle_plan -- every other plane-to-plane
    // plan that would come here)
    case kRuleGicp: break;
    }
}

// Waits (bounded) until the device has stored `want` in a host-mapped word, as `value_of` reads it out of the word.
template <class W, class F>
int await_word(icpmi_ctx *ctx, const volatile W *word, int want, F value_of, const char *never, W *out)
{
    W v = *word;
    for (long spin = 0; value_of(v) != want; ++spin) {
        if (spin > 2000000) { // ~seconds: something is wrong with the stream, find out what
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            v = *word;
            if (value_of(v) != want) return fail(ctx, ICPMI_ERR_HIP, "%s", never);
            break;
        }
        if ((spin & 63) == 63) sched_yield();
        v = *word;
    }
    *out = v;
    return ICPMI_OK;
}

// One registration on its way through align_device: the call's arguments, its plan (loop_plan.h) and what the stages hand
// each other.  The stages are the member functions below, in the order align_device calls them.
struct LoopRun {
    icpmi_ctx *ctx;
    const double *d_src, *d_tgt;
    const icpmi_config *cfg;
    GateRun *gate; // (may be null): see GateRun
    int n, m, max_hist;
    hipStream_t s;
    LoopPlan p;
    bool prepared = false;
    double *cur = nullptr, *nrm = nullptr, *hist = nullptr, *partials = nullptr;
    int *idx = nullptr;
    const double *fin_rows = nullptr; // what the step kernels sum
    IcpState *hs = nullptr, *st = nullptr; // the pinned copy; of the two device buffers the one the coming kernels read
    RowBounds rb{};
    BoundedRows lr{};
    PartialRows pr{};
    const unsigned *src_perm = nullptr;
    int pass_no = 0;                  // coarse passes queued so far: selects the work counter (see k_nn_coarse_list)
    bool pass_list = false;           // the coming bounded pass runs over the packed list (false: over every row -- a call's first pass)
    bool small_first = true;          // the small-cloud kernel's first pass applies the initial transform to the caller's rows
    std::vector<unsigned> want_known; // [p - 1]: the rows pass p wanted listed, as far as the host has read them
    std::vector<char> lean_passes;    // [p - 1]: pass p was queued lean
    bool lean_cur = false, lean_nxt = false; // the pass being queued, and the one after it
    // solo passes (solo_pass.h): the rows pass p did not find certified, as far as the host has read them; whether the tail of
    // the pass being queued is the solo kernel; whether the tail of the pass before was (this pass then launches its tail
    // only); and which of the two areas of group rows this pass's tail sums
    std::vector<unsigned> uncert_known;
    bool solo_cur = false, solo_fed = false;
    int solo_area = 0;
    // before each k_row_list for pass `next`: where it stores the rows listed and, with the match margin, the rows certified
    // for the coming pass (profiling)
    unsigned *rows_count = nullptr, *cert_count = nullptr;
    bool ended_early = false;         // the host has SEEN the device leave the loop on a convergence test
    bool counters_back = false, stats_back = false;
    int stat_passes = 0, hl = 0;
    // the call's and the loop's brackets: closed by `queue_loop` behind the last pass, or with the run
    std::optional<Range> range_call;
    std::optional<StageTimer> t_total;
    std::optional<Range> range_loop;
    std::optional<StageTimer> t_loop;

    // Stage 1: the buffers every form needs, and the start state
    int begin()
    {
        int rc;
        ctx->loop_rows = -1; // (set again once this call has completed)
        ctx->nm_valid = false;
        ctx->nm_count = 1;
        if ((rc = reserve(ctx, ctx->cur, sizeof(double) * 3 * (size_t)n))) return rc;
        if ((rc = reserve(ctx, ctx->tgt.nrm, sizeof(double) * 3 * (size_t)m))) return rc;
        if ((rc = reserve(ctx, ctx->idx, sizeof(int) * (size_t)n))) return rc;
        if ((rc = reserve(ctx, ctx->history, sizeof(double) * (size_t)(max_hist + 1)))) return rc;
        cur = (double *)ctx->cur.p;
        nrm = (double *)ctx->tgt.nrm.p;
        idx = (int *)ctx->idx.p;
        hist = (double *)ctx->history.p;
        range_call.emplace("icpmi:align");
        t_total.emplace(ctx, ST_TOTAL);
        // state: total = initial_transform (icp.hpp:163,178), prev_error = DBL_MAX (icp.hpp:179)
        hs = ctx->h_state;
        memset(hs, 0, sizeof(*hs));
        memcpy(hs->total, cfg->initial_transform, sizeof(double) * 16);
        hs->prev_error = 1.7976931348623157e308;
        hs->tolerance = cfg->tolerance;
        hs->min_error = cfg->min_error;
        hs->max_hist = max_hist;
        // two state buffers: the sharded loop's fused step + transform kernel reads one and writes the
        // other (k_step_transform); `st` is the one the coming kernels read
        st = ctx->d_state;
        HIP_TRY(ctx, hipMemcpyAsync(st, hs, sizeof(IcpState), hipMemcpyHostToDevice, s));
        return ICPMI_OK;
    }

    // Stage 1b, plane-to-plane rows only (icp_gicp.h): the source's normals, once per call, on the rows as the caller gave
    // them -- its search structure (prepare_nn) and launch_normals, as icpmi_estimate_normals runs them -- into src_nrm in
    // the caller's row order, on the call's stream and in front of the target's preparation, whose buffers it uses.  A
    // target the context remembered (prep_valid) is forgotten by it: prepare_search then builds this call's target anew.
    int source_normals()
    {
        if (!gate || !gate->gicp || n <= 0) return ICPMI_OK; // (never on a context with a communicator: validate_gicp)
        int rc;
        if ((rc = reserve(ctx, ctx->src_nrm, sizeof(double) * 3 * (size_t)n))) return rc;
        if ((rc = prepare_nn(ctx, d_src, n, n))) return rc;
        const int k = ctx->opt.normal_k;
        return launch_normals(ctx, d_src, n, k, 0, n, (double *)ctx->src_nrm.p, sorted_normal_rows(ctx, k, n), true);
    }

    // Stage 2a: the target's search structure, unless the context holds it (prepare_target)
    int prepare_search()
    {
        const bool sharded = ctx->comm != nullptr || ctx->cb_allreduce != nullptr;
        if (gate && sharded) return fail(ctx, ICPMI_ERR_ARG, "a context with a communicator does not run gated registrations");
        prepared = !sharded && ctx->tgt.prep_valid && ctx->tgt.prep_tgt == d_tgt && ctx->tgt.prep_m == m && ctx->tgt.prep_engine == engine_for(ctx, m, n);
        // (the ranks of a sharded run must agree on the engine -- it decides the order of the normal rows they gather -- so
        // there AUTO looks at the target alone, whatever this rank's share of the source)
        return prepared ? ICPMI_OK : prepare_nn(ctx, d_tgt, m, sharded ? std::max(n, kMfmaMinQueries) : n);
    }

    // Stage 2b: with the engine known, the call's form (loop_plan.h) and the partial rows it needs
    int settle_plan()
    {
        LoopFacts f = target_facts(ctx);
        f.n = n;
        f.m = m;
        f.cu_count = ctx->cu_count;
        f.normal_k = ctx->opt.normal_k;
        f.comm = ctx->comm != nullptr || ctx->cb_allreduce != nullptr;
        f.rule = rule_of(gate);
        f.gicp_small = gate && gate->gicp && gate->gicp_small;
        f.profile = ctx->opt.profile;
        f.sw_bounded = nn_bounded_enabled();
        f.sw_reuse = nn_reuse_enabled();
        f.sw_margin = nn_margin_enabled();
        f.sw_lean = nn_lean_enabled();
        f.sw_lean_from = nn_lean_from();
        f.sw_fuse_finish = fuse_finish_enabled();
        f.sw_cull_full = nn_cull_full_enabled();
        f.sw_solo = nn_solo_enabled();
        f.sw_solo_from = nn_solo_from();
        p = make_loop_plan(f);
        if (p.error) return fail(ctx, ICPMI_ERR_ARG, p.error, p.rblocks);
        int rc;
        if ((rc = reserve(ctx, ctx->partials, PartialRows(nullptr, p.rblocks, p.rblocks2, p.solo_on).bytes))) return rc;
        pr = PartialRows(ctx->partials.p, p.rblocks, p.rblocks2, p.solo_on);
        partials = pr.rows;
        fin_rows = p.sum_tree ? pr.groups[0] : partials;
        return ICPMI_OK;
    }

    // Stage 2c: normals of the target (icp.hpp:169-171).  With several ranks each computes a slice of
    // rows against the full target and the slices are all-gathered.
    int target_normals()
    {
        int rc;
        // pruned engine: rows are taken in the target's Morton order, so that a block's neighbours
        // lie in few splits (launch_normals); a rank's slice is then a range of sorted positions
        const bool sorted_rows = sorted_normal_rows(ctx, ctx->opt.normal_k, m);
        if (p.sharded) {
            int per = (m + ctx->n_ranks - 1) / ctx->n_ranks;
            if (sorted_rows) per = (per + kCoarseQueries - 1) / kCoarseQueries * kCoarseQueries; // whole blocks (and slots) per rank
            if ((rc = reserve(ctx, ctx->stage_a, sizeof(double) * 3 * (size_t)per * ctx->n_ranks))) return rc;
            double *gathered = (double *)ctx->stage_a.p;
            const int row0 = (int)std::min<long>(m, (long)ctx->rank * per), row1 = (int)std::min<long>(m, (long)row0 + per);
            // rows land at their global offset inside `gathered`, so the gather is in place
            if ((rc = launch_normals(ctx, d_tgt, m, ctx->opt.normal_k, row0, row1, gathered, sorted_rows, false))) return rc;
            if ((rc = exchange_allgather(ctx, gathered, 3 * (size_t)per))) return rc;
            if (sorted_rows)
                hipLaunchKernelGGL(k_scatter_rows, dim3((m + 255) / 256), dim3(256), 0, s, (const double *)gathered,
                                   ctx->tgt.perm(), m, nrm);
            else
                HIP_TRY(ctx, hipMemcpyAsync(nrm, gathered, sizeof(double) * 3 * (size_t)m,
                                            hipMemcpyDeviceToDevice, s));
        } else if (!prepared) {
            if ((rc = launch_normals(ctx, d_tgt, m, ctx->opt.normal_k, 0, m, nrm, sorted_rows, true))) return rc;
            if ((rc = sort_normals(ctx, m))) return rc;
        }
        ctx->tgt.prep_valid = false; // (the stream path prepares the next target below; nothing else relies on it)
        return ICPMI_OK;
    }

    // Stage 3: the Morton order of the source rows, where the plan sorts them (LoopPlan::sort_source), and the culled engine's
    // group lists
    int sort_source()
    {
        int rc;
        size_t sort_bytes = 0;
        const int bblocks = std::max(1, std::min(256, (n + 255) / 256));
        if (p.sort_source) {
            HIP_TRY(ctx, sort_pairs_u32(nullptr, &sort_bytes, nullptr, nullptr, nullptr, nullptr, (unsigned)n, s));
            if ((rc = reserve(ctx, ctx->src_sort, SortPlanes(nullptr, (size_t)n).bytes))) return rc;
            if ((rc = reserve(ctx, ctx->sort_tmp, sort_bytes))) return rc; // the target's sort is done (stream order)
            if ((rc = reserve(ctx, ctx->bbox_part, sizeof(double) * 6 * (size_t)bblocks))) return rc;
        }
        if (p.pruned || p.cull_full) { // the group lists of the coming passes (nn_culled.h); both sets of counters start empty
            if ((rc = reserve_group_lists(ctx, ctx->tgt.nn_splits, (n + kGroupRows - 1) / kGroupRows))) return rc;
            HIP_TRY(ctx, hipMemsetAsync(ctx->grp_cnt.p, 0, group_counters(ctx).bytes, s));
        }
        if (!p.sort_source) return ICPMI_OK;
        // (Measured and not kept: this dozen of small launches on a stream of its own beside the target's pre-pass and normals
        // -- 180 us off the call under rocprofv3, whose launch overhead starves the device at the head of a call, and nothing
        // without it: 8,567 against 8,595 iterations/s at C3.)
        NnFrame *sframe = ctx->tgt.source_frame();
        const SortPlanes sp(ctx->src_sort.p, (size_t)n);
        StageTimer t(ctx, ST_SETUP);
        if (n <= kBboxSingleMax)
            hipLaunchKernelGGL(k_bbox_single, dim3(1), dim3(1024), 0, s, d_src, n, sframe, 1, (unsigned long long *)nullptr);
        else {
            hipLaunchKernelGGL(k_bbox_partial, dim3(bblocks), dim3(256), 0, s, d_src, n, (double *)ctx->bbox_part.p, 1);
            hipLaunchKernelGGL(k_bbox_final, dim3(1), dim3(64), 0, s, (const double *)ctx->bbox_part.p, bblocks, sframe);
        }
        hipLaunchKernelGGL(k_morton_keys, dim3((n + 255) / 256), dim3(256), 0, s, d_src, n, (const NnFrame *)sframe,
                           sp.keys_in, sp.vals_in);
        HIP_TRY(ctx, sort_pairs_u32(ctx->sort_tmp.p, &sort_bytes, sp.keys_in, sp.keys_out, sp.vals_in, sp.perm, (unsigned)n, s));
        src_perm = sp.perm;
        return ICPMI_OK;
    }

    // Stage 4: the rows' bounds and lists of a bounded loop, the first move and the first pass's bounds
    int first_move()
    {
        int rc;
        if (p.bounded) {
            if ((rc = reserve(ctx, ctx->nn_lists, BoundedRows(nullptr, (size_t)n).bytes))) return rc;
            lr = BoundedRows(ctx->nn_lists.p, (size_t)n);
            rb = RowBounds{d_tgt, idx, m, lr.ub, lr.ubf, lr.sqf, lr.cnt};
            if (p.reuse) {
                rb.xb = lr.xb;
                rb.mask = lr.mask;
                rb.skin = kNnSkin;
                rb.loose = kNnLoose;
                if (p.margin) rb.scan = lr.scan, rb.cover = lr.cover, rb.cert = lr.cert;
                if (ctx->opt.profile) HIP_TRY(ctx, hipMemsetAsync(lr.stat_rows, 0, sizeof(unsigned) * 3 * kReuseStatPasses, s));
            }
        }
        // current_source = source * R0^T + t0^T (icp.hpp:174-176)
        if (n > 0 && !p.small) { // (an empty shard of a sharded run launches nothing over its rows; the small-cloud kernel moves them itself)
            StageTimer t(ctx, ST_TRANSFORM);
            hipLaunchKernelGGL(k_transform, dim3(std::min(2048, (n + 255) / 256)), dim3(256), 0, s, d_src, cur, n, st, 1, 0, src_perm);
            if (p.bounded) // the first pass's incumbents and bounds (and, culled engine and culled full passes, its group lists: set 0)
                hipLaunchKernelGGL(k_nn_prebound1, dim3((n + kPreThreads - 1) / kPreThreads), dim3(kPreThreads), 0, s, (const double *)cur, n, ctx->tgt.sorted(),
                                   ctx->tgt.sorted_keys(),
                                   ctx->tgt.perm(), m, ctx->tgt.nn_ms, ctx->tgt.frame(), idx, rb,
                                   ctx->tgt.split_frames(), ctx->tgt.nn_splits,
                                   p.pruned || p.cull_full ? group_lists(ctx, 0) : GroupLists{nullptr, nullptr, 0});
        }
        return ICPMI_OK;
    }

    // k_finish_step by the call's rule: the gated and robust kernels take the count from the partial rows, not from n
    void launch_finish_step(const double *rows, int blocks, int final_pass, int *progress, int ticket)
    {
        switch (p.rule) {
        case kRuleRobust: hipLaunchKernelGGL(k_finish_step_robust, dim3(1), dim3(kFinishThreads), 0, s, rows, blocks, st, hist, final_pass, progress, ticket); break;
        case kRuleGicp: // (the gate's partial row: 28 sums and the kept rows)
        case kRuleGate: hipLaunchKernelGGL(k_finish_step_gated, dim3(1), dim3(kFinishThreads), 0, s, rows, blocks, st, hist, final_pass, progress, ticket); break;
        case kRuleNone: hipLaunchKernelGGL(k_finish_step, dim3(1), dim3(kFinishThreads), 0, s, rows, blocks, n, st, hist, final_pass, progress, ticket); break;
        }
    }

    // Stage 5, one pass of a small cloud: the rows' work in one kernel (icp_small.h), then the step
    int queue_pass_small(int final_pass, int *progress, int ticket)
    {
        {
            Range range("icpmi:nn_search");
            StageTimer t(ctx, ST_NN);
            if (p.rule == kRuleGicp) // (the gated kernel's arguments, then the source's normals and the rule's two words)
                hipLaunchKernelGGL(k_icp_small_gicp, dim3(p.rblocks), dim3(kSmallThreads), 0, s,
                                   small_first ? d_src : (const double *)cur, cur, n, (const IcpState *)st, small_first ? 1 : 0, ctx->tgt.operands(),
                                   ctx->tgt.split_frames(), ctx->tgt.nn_splits, ctx->tgt.sorted(), (const double *)ctx->tgt.nrm_sorted.p,
                                   ctx->tgt.perm(), m, ctx->tgt.nn_ms, d_tgt, (const double *)nrm, partials,
                                   ctx->tgt.counters(), gate->g2, (const double *)ctx->src_nrm.p, gate->c, gate->kappa);
            else
                launch_by_rule(gate, k_icp_small, k_icp_small_gated, k_icp_small_robust, dim3(p.rblocks), dim3(kSmallThreads), s,
                               small_first ? d_src : (const double *)cur, cur, n, (const IcpState *)st, small_first ? 1 : 0, ctx->tgt.operands(),
                               ctx->tgt.split_frames(), ctx->tgt.nn_splits, ctx->tgt.sorted(), (const double *)ctx->tgt.nrm_sorted.p,
                               ctx->tgt.perm(), m, ctx->tgt.nn_ms, d_tgt, (const double *)nrm, partials,
                               ctx->tgt.counters());
            small_first = false;
            ctx->prof.nn_pairs += (double)n * (double)m;
            ctx->prof.small_launches += 1;
            ctx->prof.nn_coarse_blocks += (int64_t)((n + kCoarseQueries - 1) / kCoarseQueries) * ctx->tgt.nn_splits; // the units the general path would run
        }
        Range range("icpmi:reduce_solve");
        StageTimer t(ctx, ST_REDUCE);
        launch_finish_step(partials, p.rblocks, final_pass, progress, ticket);
        HIP_TRY(ctx, hipGetLastError());
        return ICPMI_OK;
    }

    // Lean passes: this pass (P, from 1) is what the tail of the pass before decided; the pass after it is decided now, from
    // the two latest counts the queue loop has read: want(P - 3) and want(P - 2) (lean_next, loop_plan.h)
    void decide_lean(int final_pass)
    {
        lean_cur = lean_nxt;
        lean_nxt = lean_next(pass_no + 1, final_pass, p.lean_from, want_known.data(), (int)want_known.size());
        lean_passes.push_back(lean_cur ? 1 : 0);
        if (lean_cur) ctx->prof.nn_lean_passes += 1;
    }

    // Solo passes: whether this pass (P, from 1) is fed by the solo kernel that ended the pass before, and whether its own
    // tail is one, from the two latest counts the queue loop has read (solo_next, loop_plan.h).  The pass behind a solo
    // kernel is lean (by the rule it is anyway; the test hook).
    void decide_solo(int final_pass)
    {
        solo_fed = solo_cur;
        solo_cur = solo_next(pass_no + 1, final_pass, p.solo_from, uncert_known.data(), (int)uncert_known.size());
        if (solo_cur) ctx->prof.nn_solo_passes += 1;
    }
    // the group rows this pass's tail sums, and the solo kernel's own arguments: what it writes for the coming pass and, in a
    // pass that is itself fed by one, the counts it publishes in k_sum_groups' stead (also k_publish_counts' arguments)
    const double *pass_fin_rows() const { return solo_fed ? pr.groups[solo_area] : fin_rows; }
    SoloPass solo_args() const
    {
        const int here = pass_no - 1, at = std::min(here, kReuseStatPasses - 1); // (this pass, from 0)
        const int out_area = solo_fed ? 1 - solo_area : 1;
        SoloPass sp{ctx->tgt.sorted(), ctx->tgt.perm(), ctx->tgt.nn_ms, ctx->tgt.nn_splits,
                    ctx->tgt.split_frames(), (const double *)nrm, idx, pr.groups[out_area], pr.counts[(here + 1) & 1],
                    nullptr, 0, nullptr, nullptr, 0u, n, nullptr, nullptr, nullptr};
        if (solo_fed) {
            sp.counts_in = pr.counts[here & 1];
            sp.blocks_in = p.fin_blocks;
            sp.want = ctx->d_want + ProgressRings::wanted(here % kFlagRing);
            sp.uncert = ctx->d_want + ProgressRings::uncertified(here % kFlagRing);
            sp.ticket = (unsigned)(here + 1);
            if (ctx->opt.profile) sp.stat_rows = lr.stat_rows + at, sp.stat_cert = lr.stat_cert + at, sp.stat_searched = lr.stat_searched + at;
        }
        return sp;
    }

    // ... its search: the MFMA engines' resolve leaves the partial rows too (LoopPlan::fused)
    int pass_search()
    {
        if (n <= 0) return ICPMI_OK;
        if (solo_fed) { // (the solo kernel that ended the pass before has left this pass's matches and group sums: a lean bounded pass)
            ctx->prof.bounded_launches += 1;
            return ICPMI_OK;
        }
        if (!p.fused) return launch_nn(ctx, cur, n, d_tgt, m, idx, nullptr, st);
        // (bounded: incumbents in idx, bounds in place -- from k_nn_prebound1 or the kernel that moved the rows)
        // (culled full passes: a call's first two, whichever of them is the post-loop pass)
        const NnPass pass{p.pruned ? pass_no : -1, p.bounded, pass_list, lean_cur, p.margin, p.cull_full && pass_no < 2 ? pass_no : -1};
        return launch_nn_mfma(ctx, cur, n, m, idx, nullptr, st, d_tgt, nrm, partials, pass);
    }

    // ... the partial rows of an unfused pass (k_reduce*) and, of very many rows, their sums in groups
    void pass_sums()
    {
        if (p.rule == kRuleGicp)
            hipLaunchKernelGGL(k_reduce_gicp, dim3(p.rblocks), dim3(256), 0, s, (const double *)cur, n, d_tgt, m, (const double *)nrm,
                               (const int *)idx, (const double *)ctx->src_nrm.p, partials, (const IcpState *)st, gate->g2, gate->c,
                               gate->kappa);
        else if (!p.fused)
            launch_by_rule(gate, k_reduce_rule<RuleNone>, k_reduce_rule<RuleGate, double>, k_reduce_rule<RuleRobust, double, int, double>, dim3(p.rblocks), dim3(256), s, (const double *)cur, n, d_tgt, m,
                           (const double *)nrm, (const int *)idx, partials, (const IcpState *)st);
        if (solo_fed) { // no partial rows to add; the pass's counts are the solo tail's to publish, or a wave's in front of any other
            if (!solo_cur) hipLaunchKernelGGL(k_publish_counts, dim3(1), dim3(64), 0, s, (const IcpState *)st, solo_args());
        } else if (p.sum_tree && p.lean_on) { // (+ the workgroup that counts the rows this pass wanted listed; pass_no - 1: this pass, from 0)
            const int here = pass_no - 1, at = std::min(here, kReuseStatPasses - 1);
            const bool stats = lean_cur && ctx->opt.profile;
            const WantPublish wp{ctx->d_want + ProgressRings::wanted(here % kFlagRing), (unsigned)(here + 1), n, here == 0, (const unsigned long long *)lr.mask,
                                 p.margin ? (const unsigned long long *)lr.cert : nullptr, stats ? lr.stat_rows + at : nullptr,
                                 stats && p.margin ? lr.stat_cert + at : nullptr,
                                 p.solo_on ? ctx->d_want + ProgressRings::uncertified(here % kFlagRing) : nullptr};
            hipLaunchKernelGGL(k_sum_groups, dim3((p.rblocks2 + 7) / 8 + 1), dim3(256), 0, s, (const double *)partials, p.rblocks,
                               pr.groups[0], (const IcpState *)st, wp);
        } else if (p.sum_tree)
            hipLaunchKernelGGL(k_sum_groups, dim3((p.rblocks2 + 7) / 8), dim3(256), 0, s, (const double *)partials, p.rblocks,
                               pr.groups[0], (const IcpState *)st, WantPublish{});
    }

    // ... the final sum, the exchange of a sharded run, the step and the rows' move (with their bounds, RowBounds, and the culled
    // engine's group lists of the coming pass: set pass_no & 1); behind them the coming pass's list of rows
    int pass_step_and_move(int final_pass, int *progress, int ticket)
    {
        const bool step_moves = fuse_step(p, n, final_pass), finish_moves = fuse_finish(p, n, final_pass);
        const SplitFrame *frames = ctx->tgt.split_frames();
        const int splits = ctx->tgt.nn_splits;
        IcpState *other = st == ctx->d_state ? ctx->d_state + 1 : ctx->d_state; // (the fused kernels write the other state buffer)
        if (p.sharded) {
            int rc;
            hipLaunchKernelGGL(k_finish, dim3(1), dim3(kFinishThreads), 0, s, pass_fin_rows(), p.fin_blocks, n, st);
            {
                StageTimer tx(ctx, ST_EXCHANGE); // the per-pass all-reduce alone (30 doubles; RCCL on the library's stream)
                if ((rc = exchange_allreduce(ctx, st->sums, kNumExchanged))) return rc;
            }
            if (step_moves) { // step + pose update of this rank's rows in one launch, into the other state buffer
                if (p.pruned)
                    hipLaunchKernelGGL(k_step_transform_cull, dim3(std::min(2048, (n + 255) / 256)), dim3(256), 0, s,
                                       (const double *)cur, cur, n, (const IcpState *)st, other, hist, progress, ticket,
                                       ctx->n_ranks, rb, frames, splits, group_lists(ctx, pass_no & 1));
                else
                    hipLaunchKernelGGL(k_step_transform, dim3(std::min(2048, (n + 255) / 256)), dim3(256), 0, s,
                                       (const double *)cur, cur, n, (const IcpState *)st, other, hist, progress, ticket,
                                       ctx->n_ranks, rb);
                st = other;
            } else {
                hipLaunchKernelGGL(k_step, dim3(1), dim3(64), 0, s, st, hist, final_pass, progress, ticket,
                                   ctx->n_ranks);
            }
        } else if (finish_moves) { // final sum + step + pose update of the rows in one launch
            if (solo_cur) { // (... and the coming pass's terms and group sums: solo_pass.h)
                hipLaunchKernelGGL(k_finish_step_transform_solo, dim3(finish_transform_blocks(n)), dim3(kFinishThreads), 0, s,
                                   pass_fin_rows(), p.fin_blocks, n, (const double *)cur, cur, n, (const IcpState *)st, other, hist,
                                   progress, ticket, rb, solo_args());
                solo_area = solo_fed ? 1 - solo_area : 1;
            } else if (p.pruned)
                hipLaunchKernelGGL(k_finish_step_transform_cull, dim3(finish_transform_blocks(n)), dim3(kFinishThreads), 0, s,
                                   fin_rows, p.fin_blocks, n, (const double *)cur, cur, n, (const IcpState *)st, other,
                                   hist, progress, ticket, rb, frames, splits, group_lists(ctx, pass_no & 1));
            else
                hipLaunchKernelGGL(k_finish_step_transform, dim3(finish_transform_blocks(n)), dim3(kFinishThreads), 0, s,
                                   pass_fin_rows(), p.fin_blocks, n, (const double *)cur, cur, n,
                                   (const IcpState *)st, other, hist, progress, ticket, rb);
            st = other;
        } else {
            launch_finish_step(pass_fin_rows(), p.fin_blocks, final_pass, progress, ticket);
        }
        return ICPMI_OK;
    }

    // Stage 5, one pass of the general kernels: search, sums, step and move
    int queue_pass_general(int final_pass, int *progress, int ticket)
    {
        int rc;
        if (p.lean_on) decide_lean(final_pass);
        if (p.solo_on) decide_solo(final_pass);
        if ((rc = pass_search())) return rc;
        if (n > 0 && p.fused) {
            ++pass_no;
            if (!final_pass) {
                const int at = std::min(pass_no, kReuseStatPasses - 1);
                if (p.reuse) rows_count = ctx->opt.profile ? lr.stat_rows + at : nullptr;
                if (p.margin) cert_count = ctx->opt.profile ? lr.stat_cert + at : nullptr;
            }
            pass_list = p.reuse && !final_pass;
        }
        {
            Range range("icpmi:reduce_solve");
            StageTimer t(ctx, ST_REDUCE);
            pass_sums();
            if ((rc = pass_step_and_move(final_pass, progress, ticket))) return rc;
        }
        if (!final_pass && n > 0 && !fuse_step(p, n, final_pass) && !fuse_finish(p, n, final_pass)) {
            Range range("icpmi:transform");
            StageTimer t(ctx, ST_TRANSFORM);
            if (p.pruned) // (ICPMI_FUSE_FINISH=0 only: + the rows' bounds and the group lists of the coming pass, set pass_no & 1)
                hipLaunchKernelGGL(k_transform_cull, dim3((n + 255) / 256), dim3(256), 0, s, (const double *)cur, (const unsigned *)nullptr,
                                   cur, n, (const IcpState *)st, 0, 1, rb, ctx->tgt.split_frames(), ctx->tgt.nn_splits, group_lists(ctx, pass_no & 1));
            else
                hipLaunchKernelGGL(k_transform, dim3(std::min(2048, (n + 255) / 256)), dim3(256), 0, s,
                                   cur, cur, n, st, 0, 1, (const unsigned *)nullptr, rb);
        }
        // culled full passes: the box test of the rows the first pass's mover has just left, into set 1 -- the second pass's
        // group lists (the first pass's coarse kernel has cleared that set's counters)
        if (solo_cur) lean_nxt = true; // (nothing of the coming pass but its tail is launched)
        if (p.cull_full && pass_no == 1 && !final_pass && !lean_nxt)
            hipLaunchKernelGGL(k_row_group_cull, dim3(((n + 63) / 64 + 15) / 16), dim3(1024), 0, s, (const double *)cur, n, (const float *)lr.ubf,
                               ctx->tgt.split_frames(), ctx->tgt.nn_splits, group_lists(ctx, 1), (const IcpState *)st);
        if (pass_list && !lean_nxt) // the rows just moved left their "listed again" words: the coming pass's list of rows
            hipLaunchKernelGGL(k_row_list, dim3(((n + 63) / 64 + kRowListThreads - 1) / kRowListThreads), dim3(kRowListThreads), 0, s,
                               (const unsigned long long *)lr.mask, n, lr.list, (const IcpState *)st,
                               (const unsigned long long *)(p.margin ? lr.cert : nullptr), cert_count, rows_count);
        return ICPMI_OK;
    }

    int queue_pass(int final_pass, int *progress, int ticket) // Stage 5, one pass
    {
        return p.small ? queue_pass_small(final_pass, progress, ticket) : queue_pass_general(final_pass, progress, ticket);
    }

    // Stage 5: the queue loop.  The host runs kLag passes ahead of the device's progress words.
    // `after_first` (may be null): called once the first iterations are queued and before the host first waits for
    // the device -- what it queues (on another stream) costs the host its launch time while the device is busy
    int queue_loop(int (*after_first)(icpmi_ctx *))
    {
        int rc;
        range_loop.emplace("icpmi:icp_loop");
        t_loop.emplace(ctx, ST_LOOP);
        for (int i = 0; i < ProgressRings::kProgressWords; ++i) ctx->h_flags[i] = 0;
        for (int i = 0; i < ProgressRings::kCountWords; ++i) ctx->h_want[i] = 0ull;
        bool after_first_done = after_first == nullptr;
        for (int it = 0; it < cfg->max_iterations; ++it) {
            if (it >= kLag && !after_first_done) {
                after_first_done = true;
                (void)after_first(ctx); // (a failure there only means the next call prepares its target itself)
            }
            if (it >= kLag) {
                // wait until iteration it - kLag has reported; stop queueing once the loop has ended
                const int slot = (it - kLag) % kFlagRing, want = it - kLag + 1;
                int32_t v;
                if ((rc = await_word(ctx, &ctx->h_flags[slot], want, [](int32_t x) { return (int)(x >> 1); },
                                     "device progress word never arrived", &v)))
                    return rc;
                if (v & 1) { // loop already left on the device
                    ended_early = true;
                    break;
                }
                if (p.lean_on) {
                    // the rows that iteration's pass wanted listed: its k_sum_groups ran in front of the kernel whose progress word
                    // has just been read, so the word is there or on its way (the same bounded spin)
                    unsigned long long w;
                    if ((rc = await_word(ctx, &ctx->h_want[ProgressRings::wanted(slot)], want, [](unsigned long long x) { return (int)(x >> 32); },
                                         "device row count word never arrived", &w)))
                        return rc;
                    want_known.push_back((unsigned)(w & 0xFFFFFFFFull));
                    if (p.solo_on) { // ... and the rows it did not find certified, published with it
                        if ((rc = await_word(ctx, &ctx->h_want[ProgressRings::uncertified(slot)], want, [](unsigned long long x) { return (int)(x >> 32); },
                                             "device row count word never arrived", &w)))
                            return rc;
                        uncert_known.push_back((unsigned)(w & 0xFFFFFFFFull));
                    }
                }
            }
            if ((rc = queue_pass(0, ctx->d_flags + it % kFlagRing, it + 1))) return rc;
        }
        // post-loop evaluation (icp.hpp:235-252): a full pass after exhaustion; after a convergence break it restates
        // the last error, which the step that broke the loop has already entered (step_update): nothing to queue then.
        // (Single-GPU loops only: in a sharded run `done` is agreed one exchange later, k_step.)
        if (!(ended_early && !p.sharded) && (rc = queue_pass(1, nullptr, 0))) return rc;
        if (!after_first_done) (void)after_first(ctx);
        t_loop.reset();
        t_total.reset();
        return ICPMI_OK;
    }

    // Stage 6: state and history come back behind ONE wait (the history through the pinned staging area: a
    // second, blocking copy after the wait was one more host round trip per call)
    // `before_wait` (may be null): called once everything of the registration, the copies of its results
    // included, is queued and an event behind them recorded -- what it queues runs while the host waits
    // for that event only (icpmi_stream_push prepares the next frame's target there).
    int results_back(double *error_history, int32_t history_cap, int (*before_wait)(icpmi_ctx *))
    {
        const int hcopy = std::min(max_hist, history_cap);
        if ((int)ctx->h_hist_cap < hcopy) {
            if (ctx->h_hist) (void)hipHostFree(ctx->h_hist);
            ctx->h_hist = nullptr;
            ctx->h_hist_cap = 0;
            HIP_TRY(ctx, hipHostMalloc((void **)&ctx->h_hist, sizeof(double) * (size_t)(hcopy + 64), hipHostMallocDefault));
            ctx->h_hist_cap = (size_t)hcopy + 64;
        }
        HIP_TRY(ctx, hipMemcpyAsync(hs, st, sizeof(IcpState), hipMemcpyDeviceToHost, s));
        if (hcopy > 0) HIP_TRY(ctx, hipMemcpyAsync(ctx->h_hist, hist, sizeof(double) * (size_t)hcopy, hipMemcpyDeviceToHost, s));
        // profiling: the resolve's counters come back behind the same wait, and the events are read when somebody asks
        // for the profile (icpmi_get_profile) -- a blocking copy and a dozen hipEventElapsedTime calls inside every
        // call were ~0.1 ms of host time in a 9 ms C3 call, charged to the very thing they measure
        counters_back = ctx->opt.profile && ctx->tgt.nn_engine == ICPMI_SEARCH_MFMA_BF16 && ctx->tgt.nn_misc.p;
        if (counters_back) {
            HIP_TRY(ctx, hipMemcpyAsync(ctx->h_cnt, ctx->tgt.counters(), MiscBlock::kCounterBytes, hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipMemsetAsync(ctx->tgt.counters(), 0, MiscBlock::kCounterBytes, s));
            ctx->h_cnt[3] = ctx->h_cnt[4] = 0;
            if (p.pruned) // (row group, split) pairs run / of all passes: cleared with the counters at the head of the next call
                HIP_TRY(ctx, hipMemcpyAsync(ctx->h_cnt + 3, group_counters(ctx).stats, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        }
        // ... and so do list reuse's per-pass statistics (the arrays lie one behind the other: one copy into pinned memory,
        // where a blocking copy after the wait cost the caller some 15 us)
        stats_back = p.reuse && ctx->opt.profile && pass_no > 0;
        stat_passes = std::min(pass_no, kReuseStatPasses);
        if (stats_back)
            HIP_TRY(ctx, hipMemcpyAsync(ctx->h_stat, lr.stat_rows, sizeof(unsigned) * ((size_t)(p.solo_on ? 2 : p.margin ? 1 : 0) * kReuseStatPasses + stat_passes),
                                        hipMemcpyDeviceToHost, s));
        if (before_wait && ctx->opt.profile == 0) {
            // the results are waited for through an event; what before_wait queues behind it keeps the device busy
            // while the caller digests them (with profiling on, the stage timers want the whole stream drained)
            if (!ctx->result_ready) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->result_ready, hipEventDisableTiming));
            HIP_TRY(ctx, hipEventRecord(ctx->result_ready, s));
            {   // (a failure there only means the next call prepares its target itself: it must not leave its text in
                // the error string of a call that succeeded)
                const std::string keep = ctx->err;
                if (before_wait(ctx) != ICPMI_OK) ctx->err = keep;
                ctx->trailing_work = true; // kernels of the NEXT call's target are queued behind this call's results
            }
            HIP_TRY(ctx, hipEventSynchronize(ctx->result_ready));
        } else {
            HIP_TRY(ctx, hipStreamSynchronize(s));
        }
        HIP_TRY(ctx, hipGetLastError());
        hl = std::min(hs->hist_len, max_hist);
        if (hl > 0) memcpy(error_history, ctx->h_hist, sizeof(double) * (size_t)std::min(hl, history_cap));
        return ICPMI_OK;
    }

    // Stage 7: the counters and per-pass statistics that came back, into the profile
    void account_profile()
    {
        if (counters_back) {
            ctx->prof.nn_recheck_queries += (int64_t)ctx->h_cnt[0];
            ctx->prof.nn_fallback_queries += (int64_t)ctx->h_cnt[1];
            ctx->prof.nn_pruned_blocks += (int64_t)ctx->h_cnt[2];
            ctx->prof.nn_group_pairs_run += (int64_t)ctx->h_cnt[3];
            ctx->prof.nn_group_pairs += (int64_t)ctx->h_cnt[4];
            // (the older pair of fields, in 512-row units like the all-pairs engine's)
            ctx->prof.nn_pruned_blocks += (int64_t)(ctx->h_cnt[4] - ctx->h_cnt[3]) / (kCoarseQueries / kGroupRows); // (16 tiles to a 512-row block)
        }
        ctx->reuse_rows.clear();
        ctx->reuse_blocks.clear();
        ctx->margin_rows.clear();
        if (stats_back) {
            // list reuse, per pass: the rows listed (the first pass lists all) and the workgroup columns of the coarse pass that
            // ran, ceil(rows / rows per workgroup) -- none in a lean pass, which has no coarse launch; their pairs are the pairs
            // searched, and a pass none of which ran is a skipped coarse launch
            const int np = stat_passes;
            const unsigned *stat = ctx->h_stat;
            const int per = coarse_half_units(ctx->cu_count, n, ctx->tgt.nn_splits) ? kCoarseQueries / kCoarseQT : kCoarseQueries;
            ctx->reuse_rows.assign(stat, stat + np);
            ctx->reuse_rows[0] = (unsigned)n;
            ctx->reuse_blocks.resize((size_t)np);
            for (int q = 0; q < np; ++q) {
                const bool lean = q < (int)lean_passes.size() && lean_passes[q];
                ctx->reuse_blocks[q] = lean ? 0u : (unsigned)(((long)ctx->reuse_rows[q] + per - 1) / per);
            }
            if (p.margin) { // the match margin, per pass: the rows certified (the first pass certifies none)
                ctx->margin_rows.assign(stat + kReuseStatPasses, stat + kReuseStatPasses + np);
                for (int q = 0; q < np; ++q) ctx->prof.nn_rows_certified += ctx->margin_rows[q];
                if (p.solo_on)
                    for (int q = 0; q < np; ++q) ctx->prof.nn_solo_fallback_rows += stat[2 * kReuseStatPasses + q];
            }
            for (int q = 0; q < np; ++q) {
                ctx->prof.nn_rows_listed += ctx->reuse_rows[q];
                if (q > 0) ctx->prof.nn_pairs += std::min((double)n, (double)ctx->reuse_blocks[q] * per) * (double)m;
                if (q > 0 && ctx->reuse_blocks[q] == 0) ctx->prof.nn_coarse_skipped += 1;
            }
        }
        if (ctx->ev_used > 4096) harvest_profile(ctx); // (otherwise when the profile is asked for)
    }

    // Stage 8: the caller's result, what the context remembers of the loop's rows, and the rule's own outputs
    int fill_result(icpmi_result *result)
    {
        if (hs->error)
            return fail(ctx, ICPMI_ERR_RCCL, "the ranks of this sharded run disagreed on the end of the loop "
                                             "(different icpmi_config per rank, or an exchange that is not bit-identical on every rank)");
        ctx->loop_rows = n;
        ctx->loop_idx_valid = n > 0 && !p.small;
        ctx->loop_sorted = p.sort_source;
        if (gate) {
            // A gated loop's idx holds matches of rows the gate dropped as well: loop_rows stays -1 ("no registration's rows
            // are held"), so icpmi_debug_loop_rows refuses every row count and nothing reads them as an ungated loop's.
            ctx->loop_rows = -1;
            ctx->loop_idx_valid = false;
            gate->pairs = (int64_t)hs->sums[gate->kind ? 29 : 28];
            gate->weight_sum = gate->kind ? hs->sums[28] : 0.0;
        }

        // The normal matrix of the pass that produced final_error.  Every finish kernel takes a pass's sums over only while
        // the loop has not ended (`!ls.done`: finish_step_rows, k_finish_step_transform, k_finish_step_transform_cull), and
        // the breaking and the post-loop step return in front of the solve: after a convergence break these are the
        // breaking pass's sums, after exhaustion the post-loop pass's, both at `total`, whatever was queued behind.
        {
            icpmi_normal_matrix &nm = ctx->nm;
            for (int a = 0, e = 0; a < 6; ++a)
                for (int b = a; b < 6; ++b, ++e) nm.JtJ[6 * a + b] = nm.JtJ[6 * b + a] = hs->sums[e];
            memcpy(nm.Jtb, hs->sums + 21, sizeof(double) * 6);
            nm.sum_sq = hs->sums[27];
            nm.weight = hs->sums[28];
            nm.pairs = (int64_t)hs->sums[gate && gate->kind ? 29 : 28];
            memcpy(nm.T, hs->total, sizeof(double) * 16);
            ctx->nm_valid = nm.weight > 0.0; // (a gated or robust pass that kept no row leaves no matrix)
        }
        memcpy(result->transformation, hs->total, sizeof(double) * 16); // icp.hpp:254
        result->converged = hs->converged;
        result->num_iterations = hs->hist_len - 1;                      // icp.hpp:255
        result->final_error = hs->final_error;
        result->history_len = hl;
        result->loop_iterations = hs->loops;
        return ICPMI_OK;
    }
};

// `gate` (may be null): see GateRun.  A gated registration runs the small-cloud kernel's gated form in the small regime
// and otherwise the unfused general path -- search (launch_nn), k_reduce_gated, k_finish_step_gated, k_transform -- on
// whichever engine prepare_nn chose: no fused resolve, no culling, no bounds, no list reuse, no sorted rows.
// A plane-to-plane registration (GateRun::gicp) runs that general path at every size, with k_reduce_gicp for the sums,
// behind the source's normals (LoopRun::source_normals); with GateRun::gicp_small it runs k_icp_small_gicp in the small regime.
// `before_wait`, `after_first` (may be null): see LoopRun::results_back and LoopRun::queue_loop.
int align_device(icpmi_ctx *ctx, const double *d_src, int64_t n_src64, const double *d_tgt,
                 int64_t n_tgt64, const icpmi_config *cfg, icpmi_result *result,
                 double *error_history, int32_t history_cap, int (*before_wait)(icpmi_ctx *) = nullptr,
                 int (*after_first)(icpmi_ctx *) = nullptr, GateRun *gate = nullptr)
{
    LoopRun run{ctx, d_src, d_tgt, cfg, gate, (int)n_src64, (int)n_tgt64, cfg->max_iterations + 1, ctx->stream};
    int rc;
    if ((rc = run.begin())) return rc;
    if ((rc = run.source_normals())) return rc;
    if ((rc = run.prepare_search())) return rc;
    if ((rc = run.settle_plan())) return rc;
    if ((rc = run.target_normals())) return rc;
    if ((rc = run.sort_source())) return rc;
    if ((rc = run.first_move())) return rc;
    if ((rc = run.queue_loop(after_first))) return rc;
    if ((rc = run.results_back(error_history, history_cap, before_wait))) return rc;
    run.account_profile();
    return run.fill_result(result);
}

// voxel filter on device memory -> d_out (n_out rows); see voxel.h
// `finish`: wait for the centroids before returning (the public entry points promise complete
// outputs; icpmi_stream_push queues the registration behind it on the same stream instead)
// The voxel filter's working memory: the context has one set (shared with its other stages), the prefetch
// worker another, so that it can filter the next scan on its own stream while the context registers this one.
struct VoxelScratch {
    DevBuf *bbox_part, *box, *keys, *vals, *tmp;
    size_t box_offset; // of the VoxelBox inside *box
};

// No context in here (the worker thread runs it too): a code and a static message come back.
// `deferred` (the prefetch worker; implies `finish`): nothing waits for the number of voxels in the middle -- the
// prefix sum runs over all n counts, the centroid kernel is launched for min(n, out_cap) voxels and reads the
// number itself -- and count and range flag come back behind the centroids, with the call's only wait.
// `async_out` (pinned, two words; with `deferred` only): nothing is waited for at all -- run count and range flag are
// copied there behind the centroids and the CALLER looks at them once it has waited for the stream (the prefetch
// worker: the push of the file does); *n_out is then left alone.
int voxel_filter_core(hipStream_t s, VoxelScratch vs, const double *d_pts, int n, double voxel, double *d_out, int64_t out_cap,
                      int64_t *n_out, bool finish, const char **msg, bool deferred = false, unsigned *async_out = nullptr)
{
#define VOX_TRY(call)                                   \
    do {                                                \
        const hipError_t e_ = (call);                   \
        if (e_ != hipSuccess) {                         \
            *msg = hipGetErrorString(e_);               \
            return ICPMI_ERR_HIP;                       \
        }                                               \
    } while (0)
    // key origin from the bounding box, formed on the device (k_voxel_keys)
    const int bblocks = std::max(1, std::min(256, (n + 255) / 256));
    VOX_TRY(reserve_raw(*vs.bbox_part, sizeof(double) * 6 * (size_t)bblocks));
    VOX_TRY(reserve_raw(*vs.box, vs.box_offset + 64));
    VoxelBox *box = (VoxelBox *)((char *)vs.box->p + vs.box_offset);
    static_assert(sizeof(VoxelBox) == sizeof(NnFrame) && sizeof(VoxelBox) <= 64, "k_bbox_final writes an NnFrame here");
    hipLaunchKernelGGL(k_bbox_partial, dim3(bblocks), dim3(256), 0, s, d_pts, n, (double *)vs.bbox_part->p, 0);
    hipLaunchKernelGGL(k_bbox_final, dim3(1), dim3(64), 0, s, (const double *)vs.bbox_part->p, bblocks, (NnFrame *)box);
    // keys_in | keys_out | unique ; vals_in | order | counts | offsets | runs, flag
    const size_t un = (size_t)n;
    VOX_TRY(reserve_raw(*vs.keys, sizeof(unsigned long long) * 3 * un));
    VOX_TRY(reserve_raw(*vs.vals, sizeof(unsigned) * (4 * un + 16)));
    unsigned long long *keys_in = (unsigned long long *)vs.keys->p, *keys_out = keys_in + un, *uniq = keys_in + 2 * un;
    unsigned *vals_in = (unsigned *)vs.vals->p, *order = vals_in + un, *counts = vals_in + 2 * un,
             *offsets = vals_in + 3 * un, *runs_d = vals_in + 4 * un;
    size_t b1 = 0, b2 = 0, b3 = 0;
    VOX_TRY(sort_pairs_u64(nullptr, &b1, keys_in, keys_out, vals_in, order, (unsigned)n, s));
    VOX_TRY(run_lengths_u64(nullptr, &b2, keys_out, (unsigned)n, uniq, counts, runs_d, s));
    VOX_TRY(exclusive_sum_u32(nullptr, &b3, counts, offsets, (unsigned)n, s));
    VOX_TRY(reserve_raw(*vs.tmp, std::max(b1, std::max(b2, b3))));
    VOX_TRY(hipMemsetAsync(runs_d + 1, 0, sizeof(unsigned), s)); // the flag word: k_voxel_keys ORs into it
    hipLaunchKernelGGL(k_voxel_keys, dim3((n + 255) / 256), dim3(256), 0, s, d_pts, n, voxel, (const VoxelBox *)box, runs_d + 1,
                       keys_in, vals_in);
    VOX_TRY(sort_pairs_u64(vs.tmp->p, &b1, keys_in, keys_out, vals_in, order, (unsigned)n, s));
    VOX_TRY(run_lengths_u64(vs.tmp->p, &b2, keys_out, (unsigned)n, uniq, counts, runs_d, s));
    unsigned runs_flag[2] = {0, 0};
    if (deferred) {
        const int bound = (int)std::min<int64_t>(n, out_cap);
        VOX_TRY(exclusive_sum_u32(vs.tmp->p, &b3, counts, offsets, (unsigned)n, s));
        hipLaunchKernelGGL(k_voxel_centroids, dim3((bound + 3) / 4), dim3(256), 0, s, d_pts, (const unsigned *)order,
                           (const unsigned *)offsets, (const unsigned *)counts, bound, d_out, (const unsigned *)runs_d);
        VOX_TRY(hipGetLastError());
    }
    if (deferred && async_out) {
        VOX_TRY(hipMemcpyAsync(async_out, runs_d, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        return ICPMI_OK;
    }
    VOX_TRY(hipMemcpyAsync(runs_flag, runs_d, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, s)); // the call's one round trip
    VOX_TRY(hipStreamSynchronize(s));
    if (runs_flag[1]) {
        *msg = "voxel grid spans more than 2^21 cells on an axis, or a point has a non-finite coordinate";
        return ICPMI_ERR_ARG;
    }
    const unsigned runs = runs_flag[0];
    if ((int64_t)runs > out_cap) {
        *msg = "output holds fewer rows than the filter yields";
        return ICPMI_ERR_CAPACITY;
    }
    if (!deferred) {
        VOX_TRY(exclusive_sum_u32(vs.tmp->p, &b3, counts, offsets, runs, s));
        hipLaunchKernelGGL(k_voxel_centroids, dim3((runs + 3) / 4), dim3(256), 0, s, d_pts, (const unsigned *)order,
                           (const unsigned *)offsets, (const unsigned *)counts, (int)runs, d_out);
        VOX_TRY(hipGetLastError());
        if (finish) VOX_TRY(hipStreamSynchronize(s));
    }
    *n_out = runs;
    return ICPMI_OK;
#undef VOX_TRY
}

int voxel_downsample_device(icpmi_ctx *ctx, const double *d_pts, int n, double voxel, double *d_out,
                            int64_t out_cap, int64_t *n_out, bool finish = true)
{
    hipStream_t s = ctx->stream;
    if (!(voxel > 0.0)) { // file_utils.cpp:152: returns the input unchanged
        if (out_cap < n) return fail(ctx, ICPMI_ERR_CAPACITY, "output holds %lld rows, needs %d", (long long)out_cap, n);
        HIP_TRY(ctx, hipMemcpyAsync(d_out, d_pts, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToDevice, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        *n_out = n;
        return ICPMI_OK;
    }
    // (the box has a place of its own in nn_misc: offset 0 is the search's own frame of the target)
    const VoxelScratch vs{&ctx->bbox_part, &ctx->tgt.nn_misc, &ctx->vox_keys, &ctx->vox_vals, &ctx->sort_tmp, MiscBlock::kVoxelBox};
    const char *msg = "";
    const int rc = voxel_filter_core(s, vs, d_pts, n, voxel, d_out, out_cap, n_out, finish, &msg);
    return rc == ICPMI_OK ? rc : fail(ctx, rc, "%s", msg);
}

// n cell keys (kGridNone: none) -> sorted, made unique, padded: `uniq` then holds the distinct cells in ascending
// order followed by kGridNone up to n entries, and counts[n + 1] = set_n + their number (k_grid_pad).  counts holds
// n + 16 words (run lengths, then the run count and that size).  The occupancy update and the global map's rebuild
// (icpmi_map_finish) share it.
struct GridKeySort {
    unsigned long long *keys, *sorted, *uniq;
    unsigned *counts;
    int n;
};
// the sort's scratch (ctx->sort_tmp), with room for `extra` bytes of the caller's own use of it
int grid_sort_reserve(icpmi_ctx *ctx, const GridKeySort &k, size_t extra)
{
    hipStream_t s = ctx->stream;
    size_t b1 = 0, b2 = 0;
    HIP_TRY(ctx, sort_keys_u64(nullptr, &b1, k.keys, k.sorted, (unsigned)k.n, s));
    HIP_TRY(ctx, run_lengths_u64(nullptr, &b2, k.sorted, (unsigned)k.n, k.uniq, k.counts, k.counts + k.n, s));
    return reserve(ctx, ctx->sort_tmp, std::max(b1, std::max(b2, extra)));
}
int grid_sort_queue(icpmi_ctx *ctx, const GridKeySort &k, unsigned set_n)
{
    hipStream_t s = ctx->stream;
    const int n = k.n;
    unsigned *runs_d = k.counts + n, *count_d = runs_d + 1;
    size_t b1 = 0, b2 = 0;
    HIP_TRY(ctx, sort_keys_u64(nullptr, &b1, k.keys, k.sorted, (unsigned)n, s));
    HIP_TRY(ctx, run_lengths_u64(nullptr, &b2, k.sorted, (unsigned)n, k.uniq, k.counts, runs_d, s));
    HIP_TRY(ctx, sort_keys_u64(ctx->sort_tmp.p, &b1, k.keys, k.sorted, (unsigned)n, s));
    HIP_TRY(ctx, run_lengths_u64(ctx->sort_tmp.p, &b2, k.sorted, (unsigned)n, k.uniq, k.counts, runs_d, s));
    hipLaunchKernelGGL(k_grid_pad, dim3((n + 255) / 256), dim3(256), 0, s, k.uniq, n, (const unsigned *)runs_d, set_n, count_d);
    return ICPMI_OK;
}

// update_occupancy_grid (slam_node.cpp:211-221) on device memory: the frame's keys, less those the set already
// holds, sorted, made unique and merged into the set (occupancy.h); the set's new size is queued for the host
// (ctx->h_grid[0]) and picked up by grid_finish after the caller's wait.
int grid_update_queue(icpmi_ctx *ctx, const double *d_world, int n, const double sensor[3], const icpmi_grid_config *grid)
{
    if (!(grid->resolution > 0.0)) return fail(ctx, ICPMI_ERR_ARG, "grid resolution must be positive");
    hipStream_t s = ctx->stream;
    int rc;
    const size_t set_n = (size_t)ctx->grid_n, total = set_n + (size_t)n;
    if (total > (size_t)2000000000) return fail(ctx, ICPMI_ERR_ARG, "occupancy set too large");
    if (n <= 0) { // nothing to insert
        ctx->h_grid[0] = (unsigned)set_n;
        return ICPMI_OK;
    }
    const size_t un = (size_t)n;
    // grid_in: the frame's keys | sorted | unique ; grid_cnt: run lengths | runs, count ; grid_out: the merged set
    if ((rc = reserve(ctx, ctx->grid_in, sizeof(unsigned long long) * 3 * un))) return rc;
    if ((rc = reserve(ctx, ctx->grid_cnt, sizeof(unsigned) * (un + 16)))) return rc;
    if ((rc = reserve(ctx, ctx->grid_out, sizeof(unsigned long long) * total))) return rc;
    unsigned long long *keys = (unsigned long long *)ctx->grid_in.p, *sorted = keys + un, *uniq = keys + 2 * un;
    unsigned *counts = (unsigned *)ctx->grid_cnt.p;
    size_t b3 = 0;
    HIP_TRY(ctx, merge_keys_u64(nullptr, &b3, (const unsigned long long *)ctx->grid_set.p, uniq, (unsigned long long *)ctx->grid_out.p,
                                (unsigned)set_n, (unsigned)n, s));
    GridKeySort ks{keys, sorted, uniq, counts, n};
    if ((rc = grid_sort_reserve(ctx, ks, b3))) return rc;
    GridParams g{sensor[0], sensor[1], grid->resolution, grid->height_min, grid->height_max, grid->max_range};
    hipLaunchKernelGGL(k_grid_keys, dim3((n + 255) / 256), dim3(256), 0, s, d_world, n, g, keys);
    if (set_n > 0)
        hipLaunchKernelGGL(k_grid_drop_known, dim3((n + 255) / 256), dim3(256), 0, s, keys, n,
                           (const unsigned long long *)ctx->grid_set.p, (int)set_n);
    if ((rc = grid_sort_queue(ctx, ks, (unsigned)set_n))) return rc;
    unsigned *count_d = ks.counts + un + 1;
    HIP_TRY(ctx, merge_keys_u64(ctx->sort_tmp.p, &b3, set_n > 0 ? (const unsigned long long *)ctx->grid_set.p : uniq, uniq,
                                (unsigned long long *)ctx->grid_out.p, (unsigned)set_n, (unsigned)n, s));
    std::swap(ctx->grid_set, ctx->grid_out); // the merged array (cells, then n - new entries of kGridNone) is the set now
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_grid, count_d, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}
// after the stream has been waited for
void grid_finish(icpmi_ctx *ctx) { ctx->grid_n = (int64_t)ctx->h_grid[0]; }

int validate_align(icpmi_ctx *ctx, const void *src, int64_t n_src, const void *tgt, int64_t n_tgt,
                   const icpmi_config *cfg, icpmi_result *result, double *hist, int32_t cap)
{
    if (!ctx) return ICPMI_ERR_NULL;
    if (!tgt || !cfg || !result || !hist || (!src && n_src != 0)) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    // a rank of a sharded run may hold an empty shard (fewer source points than ranks, uneven
    // sharding): it contributes zero sums and a zero count and takes part in every exchange
    const bool may_be_empty = ctx->n_ranks > 1 && (ctx->comm != nullptr || ctx->cb_allreduce != nullptr);
    if (n_src < 0 || (n_src == 0 && !may_be_empty)) return fail(ctx, ICPMI_ERR_EMPTY_SOURCE, "empty source cloud");
    if (n_tgt <= 0) return fail(ctx, ICPMI_ERR_EMPTY_TARGET, "empty target cloud");
    if (n_src > (int64_t)700000000 || n_tgt > (int64_t)700000000)
        return fail(ctx, ICPMI_ERR_ARG, "cloud larger than 7e8 points");
    if (cfg->max_iterations < 0) return fail(ctx, ICPMI_ERR_ARG, "max_iterations < 0");
    if (cap < cfg->max_iterations + 1)
        return fail(ctx, ICPMI_ERR_CAPACITY, "error_history holds %d entries, needs %d", cap,
                    cfg->max_iterations + 1);
    return ICPMI_OK;
}

} // namespace

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" {

const char *icpmi_version(void) { return "icp_mi355x 0.1 (gfx950)"; }

void icpmi_options_default(icpmi_options *opt)
{
    if (!opt) return;
    opt->device = 0;
    opt->normal_k = 20; // icp.hpp:170
    opt->search = ICPMI_SEARCH_AUTO;
    opt->profile = 0;
    // a drop-in caller (slam_icp_adapter.hpp) never sees the options: let the environment pick
    // the engine.  Values outside 0..3 are ignored.
    if (const char *e = getenv("ICPMI_SEARCH")) {
        char *end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end != e && *end == '\0' && v >= ICPMI_SEARCH_AUTO && v <= ICPMI_SEARCH_MFMA_PRUNED) opt->search = (int32_t)v;
    }
}

void icpmi_config_default(icpmi_config *cfg)
{
    if (!cfg) return;
    cfg->max_iterations = 50; // types.hpp:144
    cfg->reserved = 0;
    cfg->tolerance = 1e-6;    // types.hpp:145
    cfg->min_error = 1e-9;    // types.hpp:146
    for (int i = 0; i < 16; ++i) cfg->initial_transform[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

int icpmi_create(const icpmi_options *opt, icpmi_ctx **out)
{
    if (!out) return fail(nullptr, ICPMI_ERR_NULL, "out is NULL");
    *out = nullptr;
    icpmi_options o;
    if (opt) o = *opt;
    else icpmi_options_default(&o);
    if (o.normal_k < 1 || o.normal_k > 64)
        return fail(nullptr, ICPMI_ERR_ARG, "normal_k %d outside [1,64]", o.normal_k);
    if (o.search < ICPMI_SEARCH_AUTO || o.search > ICPMI_SEARCH_MFMA_PRUNED)
        return fail(nullptr, ICPMI_ERR_ARG, "search %d is not an ICPMI_SEARCH_* value", o.search);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(nullptr, ICPMI_ERR_NO_DEVICE, "no HIP device visible");
    if (o.device < 0 || o.device >= count)
        return fail(nullptr, ICPMI_ERR_ARG, "device %d outside [0,%d)", o.device, count);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, o.device) != hipSuccess)
        return fail(nullptr, ICPMI_ERR_HIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, ICPMI_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 code only",
                    o.device, prop.gcnArchName);
    icpmi_ctx *ctx = new icpmi_ctx();
    ctx->opt = o;
    ctx->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    memset(&ctx->prof, 0, sizeof(ctx->prof));
    auto bail = [&](const char *what) {
        g_create_error = std::string(what) + ": " + hipGetErrorString(hipGetLastError());
        icpmi_destroy(ctx);
        return ICPMI_ERR_HIP;
    };
    if (hipSetDevice(o.device) != hipSuccess) return bail("hipSetDevice");
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) return bail("hipStreamCreate");
    if (hipMalloc((void **)&ctx->d_state, 2 * sizeof(IcpState)) != hipSuccess) return bail("hipMalloc state");
    if (hipHostMalloc((void **)&ctx->h_state, sizeof(IcpState), hipHostMallocDefault) != hipSuccess) return bail("hipHostMalloc");
    if (hipHostMalloc((void **)&ctx->h_flags, sizeof(int32_t) * ProgressRings::kProgressWords, hipHostMallocMapped) != hipSuccess) return bail("hipHostMalloc");
    if (hipHostMalloc((void **)&ctx->h_grid, 4 * sizeof(unsigned), hipHostMallocDefault) != hipSuccess) return bail("hipHostMalloc");
    if (hipHostMalloc((void **)&ctx->h_cnt, 8 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) return bail("hipHostMalloc");
    if (hipHostMalloc((void **)&ctx->h_want, sizeof(unsigned long long) * ProgressRings::kCountWords, hipHostMallocMapped) != hipSuccess) return bail("hipHostMalloc");
    if (hipHostMalloc((void **)&ctx->h_stat, sizeof(unsigned) * 3 * kReuseStatPasses, hipHostMallocDefault) != hipSuccess) return bail("hipHostMalloc");
    memset(ctx->h_flags, 0, sizeof(int32_t) * ProgressRings::kProgressWords);
    memset(ctx->h_want, 0, sizeof(unsigned long long) * ProgressRings::kCountWords);
    if (hipHostGetDevicePointer((void **)&ctx->d_flags, ctx->h_flags, 0) != hipSuccess) return bail("hipHostGetDevicePointer");
    if (hipHostGetDevicePointer((void **)&ctx->d_want, ctx->h_want, 0) != hipSuccess) return bail("hipHostGetDevicePointer");
    *out = ctx;
    return ICPMI_OK;
}

void icpmi_destroy(icpmi_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->opt.device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (FilePrefetch *pf = ctx->prefetch) {
        {
            std::lock_guard<std::mutex> lk(pf->mu);
            pf->quit = true;
        }
        pf->cv.notify_all();
        if (pf->worker.joinable()) pf->worker.join();
        if (getenv("ICPMI_PREFETCH_STATS") && pf->files > 0)
            fprintf(stderr, "prefetch worker, ms per file over %ld files: wait for slot %.4f, open + read (first half on its way) %.4f, queueing %.4f, filter + wait %.4f\n",
                    pf->files, pf->t_wait / pf->files, pf->t_read / pf->files, pf->t_upload / pf->files, pf->t_filter / pf->files);
        if (pf->stream) (void)hipStreamSynchronize(pf->stream);
        if (pf->h_runs) (void)hipHostFree(pf->h_runs);
        for (int k = 0; k < 2; ++k) {
            if (pf->h_buf[k]) (void)hipHostFree(pf->h_buf[k]);
            if (pf->filled[k]) (void)hipEventDestroy(pf->filled[k]);
            if (pf->d_f32[k]) (void)hipFree(pf->d_f32[k]);
            if (pf->d_raw[k]) (void)hipFree(pf->d_raw[k]);
        }
        if (pf->stream) (void)hipStreamDestroy(pf->stream);
        for (int k = 0; k < 2; ++k)
            if (pf->slot_done[k]) (void)hipEventDestroy(pf->slot_done[k]);
        for (DevBuf *b : {&pf->filtered[0], &pf->filtered[1], &pf->sc_bbox, &pf->sc_box, &pf->sc_keys, &pf->sc_vals, &pf->sc_tmp})
            release(*b);
        delete pf;
        ctx->prefetch = nullptr;
    }
    if (getenv("ICPMI_STREAM_STATS") && ctx->pushes > 0)
        fprintf(stderr, "frame stream, calling thread, ms per push over %ld pushes (the first ones carry the allocations): whole push %.4f, of it "
                        "waiting for the prefetched file %.4f, registration call %.4f (of it queueing the next target's preparation %.4f)\n",
                ctx->pushes, ctx->t_push / ctx->pushes, ctx->t_wait_file / ctx->pushes, ctx->t_align / ctx->pushes, ctx->t_prep_queue / ctx->pushes);
    if (getenv("ICPMI_STREAM_STATS") && ctx->pushes > 0) fprintf(stderr, "  device span of the registration (events on the context's stream): %.4f ms per push\n", ctx->t_gpu_span / ctx->pushes);
    if (ctx->prep_helper) icpmi_destroy(ctx->prep_helper);
    ctx->prep_helper = nullptr;
    if (ctx->prep_done) (void)hipEventDestroy(ctx->prep_done);
    if (ctx->scan_ready) (void)hipEventDestroy(ctx->scan_ready);
    for (BatchWorker *w : ctx->helpers) {
        {
            std::lock_guard<std::mutex> lk(w->mu);
            w->quit = true;
        }
        w->cv.notify_all();
        if (w->th.joinable()) w->th.join();
        icpmi_destroy(w->helper);
        delete w;
    }
    ctx->helpers.clear();
    if (ctx->comm && ctx->rccl.CommDestroy) ctx->rccl.CommDestroy(ctx->comm);
    for (DevBuf *b : {&ctx->cur, &ctx->tgt.nrm, &ctx->idx, &ctx->part_d2, &ctx->part_idx, &ctx->partials,
                      &ctx->history, &ctx->stage_a, &ctx->stage_b, &ctx->stage_c, &ctx->d2out, &ctx->src_sort, &ctx->grp_cnt, &ctx->grp_items,
                      &ctx->tgt.bpack, &ctx->coarse, &ctx->bbox_part, &ctx->tgt.nn_misc, &ctx->knn_idx, &ctx->slotmin, &ctx->nn_lists, &ctx->tgt.nrm_sorted,
                      &ctx->src_nrm, &ctx->fb_list, &ctx->tgt.sort_keys, &ctx->sort_tmp, &ctx->tgt.tgt_sorted, &ctx->tgt.frames, &ctx->vox_keys,
                      &ctx->vox_vals, &ctx->vox_out, &ctx->stream_prev, &ctx->stream_cur, &ctx->f32_stage, &ctx->deskew_raw, &ctx->deskew_times, &ctx->grid_set,
                      &ctx->grid_in, &ctx->grid_out, &ctx->grid_cnt, &ctx->world})
        release(*b);
    if (ctx->h_grid) (void)hipHostFree(ctx->h_grid);
    if (ctx->h_cnt) (void)hipHostFree(ctx->h_cnt);
    if (ctx->result_ready) (void)hipEventDestroy(ctx->result_ready);
    if (ctx->d_state) (void)hipFree(ctx->d_state);
    if (ctx->h_state) (void)hipHostFree(ctx->h_state);
    if (ctx->h_hist) (void)hipHostFree(ctx->h_hist);
    if (ctx->h_file) (void)hipHostFree(ctx->h_file);
    if (ctx->h_flags) (void)hipHostFree(ctx->h_flags);
    if (ctx->h_want) (void)hipHostFree(ctx->h_want);
    if (ctx->h_stat) (void)hipHostFree(ctx->h_stat);
    for (EventPair &p : ctx->ev_pool) {
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *icpmi_last_error(const icpmi_ctx *ctx)
{
    return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

namespace {

// the gate of the gated entry points: finite and > 0, and not on a context with a communicator (out of scope)
int validate_gate(icpmi_ctx *ctx, const icpmi_gate *gate, GateRun *run)
{
    if (!gate) return fail(ctx, ICPMI_ERR_NULL, "gate is NULL (ungated: icpmi_align*)");
    if (!(gate->max_distance > 0.0) || !std::isfinite(gate->max_distance))
        return fail(ctx, ICPMI_ERR_ARG, "max_distance must be finite and > 0");
    if (ctx->comm || ctx->cb_allreduce) return fail(ctx, ICPMI_ERR_ARG, "a context with a communicator does not run gated registrations");
    run->g2 = gate->max_distance * gate->max_distance;
    run->pairs = 0;
    return ICPMI_OK;
}

// the rule of the robust entry points (icp_robust.h) -> the run
int validate_robust(icpmi_ctx *ctx, const icpmi_robust *rule, GateRun *run)
{
    if (!rule) return fail(ctx, ICPMI_ERR_NULL, "rule is NULL (no weights: icpmi_align*)");
    if (rule->kind != ICPMI_ROBUST_HUBER && rule->kind != ICPMI_ROBUST_GEMAN_MCCLURE)
        return fail(ctx, ICPMI_ERR_ARG, "kind %d is neither ICPMI_ROBUST_HUBER nor ICPMI_ROBUST_GEMAN_MCCLURE", (int)rule->kind);
    if (!(rule->scale > 0.0) || !std::isfinite(rule->scale)) return fail(ctx, ICPMI_ERR_ARG, "scale must be finite and > 0");
    if (rule->max_distance != 0.0 && (!(rule->max_distance > 0.0) || !std::isfinite(rule->max_distance)))
        return fail(ctx, ICPMI_ERR_ARG, "max_distance must be 0 (no gate) or finite and > 0");
    if (ctx->comm || ctx->cb_allreduce) return fail(ctx, ICPMI_ERR_ARG, "a context with a communicator does not run robust registrations");
    run->g2 = rule->max_distance != 0.0 ? rule->max_distance * rule->max_distance : 1.7976931348623157e308;
    run->pairs = 0;
    run->kind = rule->kind;
    run->ks = rule->kind == ICPMI_ROBUST_GEMAN_MCCLURE ? rule->scale * rule->scale : rule->scale;
    run->weight_sum = 0.0;
    return ICPMI_OK;
}

// the rule of the plane-to-plane entry points (icp_gicp.h) -> the run
int validate_gicp(icpmi_ctx *ctx, const icpmi_gicp *rule, GateRun *run)
{
    if (!rule) return fail(ctx, ICPMI_ERR_NULL, "rule is NULL (point-to-plane: icpmi_align*)");
    if (!(rule->epsilon > 0.0 && rule->epsilon <= 1.0)) return fail(ctx, ICPMI_ERR_ARG, "epsilon must be finite with 0 < epsilon <= 1");
    if (rule->max_distance != 0.0 && (!(rule->max_distance > 0.0) || !std::isfinite(rule->max_distance)))
        return fail(ctx, ICPMI_ERR_ARG, "max_distance must be 0 (no gate) or finite and > 0");
    if (ctx->comm || ctx->cb_allreduce) return fail(ctx, ICPMI_ERR_ARG, "a context with a communicator does not run plane-to-plane registrations");
    *run = GateRun{};
    run->g2 = rule->max_distance != 0.0 ? rule->max_distance * rule->max_distance : 1.7976931348623157e308;
    run->pairs = 0;
    run->gicp = true;
    run->c = 1.0 - rule->epsilon;
    run->kappa = 2.0 * rule->epsilon;
    run->gicp_small = (rule->reserved & ICPMI_GICP_FORM_SMALL) != 0;
    return ICPMI_OK;
}

// icpmi_align after its checks: the rows (host or device memory, `kind`) go into the context's own buffers first, so
// every registration reads its clouds from the same place whoever supplied them (icpmi_align, the loop store's
// verifications).
int align_staged(icpmi_ctx *ctx, const double *source_xyz, int64_t n_src, const double *target_xyz, int64_t n_tgt,
                 hipMemcpyKind kind, const icpmi_config *cfg, icpmi_result *result, double *error_history,
                 int32_t history_cap, GateRun *gate = nullptr)
{
    int rc;
    if ((rc = reserve(ctx, ctx->stage_b, sizeof(double) * 3 * (size_t)n_src))) return rc;
    if ((rc = reserve(ctx, ctx->stage_c, sizeof(double) * 3 * (size_t)n_tgt))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_b.p, source_xyz, sizeof(double) * 3 * (size_t)n_src, kind, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_c.p, target_xyz, sizeof(double) * 3 * (size_t)n_tgt, kind, ctx->stream));
    return align_device(ctx, (const double *)ctx->stage_b.p, n_src, (const double *)ctx->stage_c.p,
                        n_tgt, cfg, result, error_history, history_cap, nullptr, nullptr, gate);
}

// Runs job(c, k) for k in [0, count) side by side: k = 0 on ctx itself, k >= 1 on helper k - 1's context and host
// thread.  status[k] receives each job's return; the first failing one is returned, with its text in ctx.
int batch_run(icpmi_ctx *ctx, int32_t count, const std::function<int(icpmi_ctx *, int)> &job, int32_t *status)
{
    int rc;
    while ((int)ctx->helpers.size() < count - 1) { // grown once, kept: their workspaces are grow-only like ctx's own
        icpmi_options o = ctx->opt;
        o.profile = 0;
        icpmi_ctx *h = nullptr;
        if ((rc = icpmi_create(&o, &h))) return fail(ctx, rc, "helper context: %s", icpmi_last_error(nullptr));
        BatchWorker *w = new BatchWorker();
        w->helper = h;
        w->th = std::thread([w] {
            std::unique_lock<std::mutex> lk(w->mu);
            for (;;) {
                w->cv.wait(lk, [w] { return w->quit || w->has_job; });
                if (w->quit) return;
                lk.unlock();
                w->job();
                lk.lock();
                w->has_job = false;
                w->done = true;
                w->cv.notify_all();
            }
        });
        ctx->helpers.push_back(w);
    }
    auto run = [&](int k) { status[k] = job(k == 0 ? ctx : ctx->helpers[(size_t)k - 1]->helper, k); };
    for (int k = 1; k < count; ++k) {
        BatchWorker *w = ctx->helpers[(size_t)k - 1];
        {
            std::lock_guard<std::mutex> lk(w->mu);
            w->job = [&run, k] { run(k); };
            w->done = false;
            w->has_job = true;
        }
        w->cv.notify_all();
    }
    run(0);
    for (int k = 1; k < count; ++k) {
        BatchWorker *w = ctx->helpers[(size_t)k - 1];
        std::unique_lock<std::mutex> lk(w->mu);
        w->cv.wait(lk, [w] { return w->done; });
    }
    ctx->nm_count = count; // (icpmi_last_normal_matrix: problem k's record is on the context that ran it)
    for (int k = 0; k < count; ++k)
        if (status[k] != ICPMI_OK) {
            if (k > 0) ctx->err = ctx->helpers[(size_t)k - 1]->helper->err;
            return status[k];
        }
    return ICPMI_OK;
}

// Every icpmi_align* entry point: the checks in their order -- the call's arguments, the context, then the entry's rule
// (`entry`: which of icpmi_gate / icpmi_robust / icpmi_gicp `rule` points to, and of icpmi_gate_info / icpmi_robust_info /
// icpmi_gicp_info `info`, which may be null; kRuleNone: neither) -- then the registration, on rows in device memory or on the caller's host arrays.
int align_entry(icpmi_ctx *ctx, bool on_device, const double *source_xyz, int64_t n_src, const double *target_xyz, int64_t n_tgt,
                const icpmi_config *cfg, LoopRule entry, const void *rule, void *info, icpmi_result *result, double *error_history,
                int32_t history_cap)
{
    int rc = validate_align(ctx, source_xyz, n_src, target_xyz, n_tgt, cfg, result, error_history, history_cap);
    if (rc) return rc;
    if ((rc = check_common(ctx))) return rc;
    GateRun run;
    if (entry == kRuleGate && (rc = validate_gate(ctx, (const icpmi_gate *)rule, &run))) return rc;
    if (entry == kRuleRobust && (rc = validate_robust(ctx, (const icpmi_robust *)rule, &run))) return rc;
    if (entry == kRuleGicp && (rc = validate_gicp(ctx, (const icpmi_gicp *)rule, &run))) return rc;
    GateRun *gate = entry == kRuleNone ? nullptr : &run;
    rc = on_device ? align_device(ctx, source_xyz, n_src, target_xyz, n_tgt, cfg, result, error_history, history_cap, nullptr, nullptr, gate)
                   : align_staged(ctx, source_xyz, n_src, target_xyz, n_tgt, hipMemcpyHostToDevice, cfg, result, error_history, history_cap, gate);
    if (rc || !info) return rc;
    if (entry == kRuleGate) *(icpmi_gate_info *)info = icpmi_gate_info{run.pairs, n_src};
    if (entry == kRuleRobust) *(icpmi_robust_info *)info = icpmi_robust_info{run.weight_sum, run.pairs, n_src};
    if (entry == kRuleGicp) *(icpmi_gicp_info *)info = icpmi_gicp_info{run.pairs, n_src};
    return ICPMI_OK;
}

// the three batch forms' own checks; `all_given`: none of the form's required arrays is null
int batch_check(icpmi_ctx *ctx, int32_t count, bool all_given)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!all_given) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (count < 1 || count > ICPMI_MAX_BATCH) return fail(ctx, ICPMI_ERR_ARG, "count %d outside [1,%d]", count, ICPMI_MAX_BATCH);
    if (ctx->comm || ctx->cb_allreduce) return fail(ctx, ICPMI_ERR_ARG, "a context with a communicator registers one (sharded) problem at a time");
    return ICPMI_OK;
}

} // namespace

int icpmi_align_device(icpmi_ctx *ctx, const double *d_source_xyz, int64_t n_src,
                       const double *d_target_xyz, int64_t n_tgt, const icpmi_config *cfg,
                       icpmi_result *result, double *error_history, int32_t history_cap)
{
    return align_entry(ctx, true, d_source_xyz, n_src, d_target_xyz, n_tgt, cfg, kRuleNone, nullptr, nullptr, result, error_history, history_cap);
}

int icpmi_align(icpmi_ctx *ctx, const double *source_xyz, int64_t n_src, const double *target_xyz,
                int64_t n_tgt, const icpmi_config *cfg, icpmi_result *result,
                double *error_history, int32_t history_cap)
{
    return align_entry(ctx, false, source_xyz, n_src, target_xyz, n_tgt, cfg, kRuleNone, nullptr, nullptr, result, error_history, history_cap);
}

int icpmi_align_batch(icpmi_ctx *ctx, int32_t count, const double *const *sources_xyz, const int64_t *n_src,
                      const double *const *targets_xyz, const int64_t *n_tgt, const icpmi_config *cfgs,
                      icpmi_result *results, double *error_history, int32_t history_stride, int32_t *status)
{
    int rc;
    if ((rc = batch_check(ctx, count, sources_xyz && n_src && targets_xyz && n_tgt && cfgs && results && error_history && status))) return rc;
    return batch_run(ctx, count, [&](icpmi_ctx *c, int k) {
        return icpmi_align(c, sources_xyz[k], n_src[k], targets_xyz[k], n_tgt[k], &cfgs[k], &results[k],
                           error_history + (size_t)k * (size_t)history_stride, history_stride);
    }, status);
}

int icpmi_align_gated_device(icpmi_ctx *ctx, const double *d_source_xyz, int64_t n_src, const double *d_target_xyz,
                             int64_t n_tgt, const icpmi_config *cfg, const icpmi_gate *gate, icpmi_result *result,
                             icpmi_gate_info *info, double *error_history, int32_t history_cap)
{
    return align_entry(ctx, true, d_source_xyz, n_src, d_target_xyz, n_tgt, cfg, kRuleGate, gate, info, result, error_history, history_cap);
}

int icpmi_align_gated(icpmi_ctx *ctx, const double *source_xyz, int64_t n_src, const double *target_xyz, int64_t n_tgt,
                      const icpmi_config *cfg, const icpmi_gate *gate, icpmi_result *result, icpmi_gate_info *info,
                      double *error_history, int32_t history_cap)
{
    return align_entry(ctx, false, source_xyz, n_src, target_xyz, n_tgt, cfg, kRuleGate, gate, info, result, error_history, history_cap);
}

int icpmi_align_gated_batch(icpmi_ctx *ctx, int32_t count, const double *const *sources_xyz, const int64_t *n_src,
                            const double *const *targets_xyz, const int64_t *n_tgt, const icpmi_config *cfgs,
                            const icpmi_gate *gates, icpmi_result *results, icpmi_gate_info *infos, double *error_history,
                            int32_t history_stride, int32_t *status)
{
    int rc;
    if ((rc = batch_check(ctx, count, sources_xyz && n_src && targets_xyz && n_tgt && cfgs && gates && results && error_history && status))) return rc;
    return batch_run(ctx, count, [&](icpmi_ctx *c, int k) {
        return icpmi_align_gated(c, sources_xyz[k], n_src[k], targets_xyz[k], n_tgt[k], &cfgs[k], &gates[k], &results[k],
                                 infos ? &infos[k] : nullptr, error_history + (size_t)k * (size_t)history_stride, history_stride);
    }, status);
}

int icpmi_align_robust_device(icpmi_ctx *ctx, const double *d_source_xyz, int64_t n_src, const double *d_target_xyz,
                              int64_t n_tgt, const icpmi_config *cfg, const icpmi_robust *rule, icpmi_result *result,
                              icpmi_robust_info *info, double *error_history, int32_t history_cap)
{
    return align_entry(ctx, true, d_source_xyz, n_src, d_target_xyz, n_tgt, cfg, kRuleRobust, rule, info, result, error_history, history_cap);
}

int icpmi_align_robust(icpmi_ctx *ctx, const double *source_xyz, int64_t n_src, const double *target_xyz, int64_t n_tgt,
                       const icpmi_config *cfg, const icpmi_robust *rule, icpmi_result *result, icpmi_robust_info *info,
                       double *error_history, int32_t history_cap)
{
    return align_entry(ctx, false, source_xyz, n_src, target_xyz, n_tgt, cfg, kRuleRobust, rule, info, result, error_history, history_cap);
}

int icpmi_align_gicp_device(icpmi_ctx *ctx, const double *d_source_xyz, int64_t n_src, const double *d_target_xyz,
                            int64_t n_tgt, const icpmi_config *cfg, const icpmi_gicp *rule, icpmi_result *result,
                            icpmi_gicp_info *info, double *error_history, int32_t history_cap)
{
    return align_entry(ctx, true, d_source_xyz, n_src, d_target_xyz, n_tgt, cfg, kRuleGicp, rule, info, result, error_history, history_cap);
}

int icpmi_align_gicp(icpmi_ctx *ctx, const double *source_xyz, int64_t n_src, const double *target_xyz, int64_t n_tgt,
                     const icpmi_config *cfg, const icpmi_gicp *rule, icpmi_result *result, icpmi_gicp_info *info,
                     double *error_history, int32_t history_cap)
{
    return align_entry(ctx, false, source_xyz, n_src, target_xyz, n_tgt, cfg, kRuleGicp, rule, info, result, error_history, history_cap);
}

int icpmi_align_gicp_batch(icpmi_ctx *ctx, int32_t count, const double *const *sources_xyz, const int64_t *n_src,
                           const double *const *targets_xyz, const int64_t *n_tgt, const icpmi_config *cfgs,
                           const icpmi_gicp *rules, icpmi_result *results, icpmi_gicp_info *infos,
                           double *error_history, int32_t history_stride, int32_t *status)
{
    int rc;
    if ((rc = batch_check(ctx, count, sources_xyz && n_src && targets_xyz && n_tgt && cfgs && rules && results && error_history && status))) return rc;
    return batch_run(ctx, count, [&](icpmi_ctx *c, int k) {
        return icpmi_align_gicp(c, sources_xyz[k], n_src[k], targets_xyz[k], n_tgt[k], &cfgs[k], &rules[k], &results[k],
                                infos ? &infos[k] : nullptr, error_history + (size_t)k * (size_t)history_stride, history_stride);
    }, status);
}

int icpmi_align_robust_batch(icpmi_ctx *ctx, int32_t count, const double *const *sources_xyz, const int64_t *n_src,
                             const double *const *targets_xyz, const int64_t *n_tgt, const icpmi_config *cfgs,
                             const icpmi_robust *rules, icpmi_result *results, icpmi_robust_info *infos,
                             double *error_history, int32_t history_stride, int32_t *status)
{
    int rc;
    if ((rc = batch_check(ctx, count, sources_xyz && n_src && targets_xyz && n_tgt && cfgs && rules && results && error_history && status))) return rc;
    return batch_run(ctx, count, [&](icpmi_ctx *c, int k) {
        return icpmi_align_robust(c, sources_xyz[k], n_src[k], targets_xyz[k], n_tgt[k], &cfgs[k], &rules[k], &results[k],
                                  infos ? &infos[k] : nullptr, error_history + (size_t)k * (size_t)history_stride, history_stride);
    }, status);
}

int icpmi_last_normal_matrix(icpmi_ctx *ctx, int32_t k, icpmi_normal_matrix *out)
{
    if (!ctx) return ICPMI_ERR_NULL;
    if (!out) return fail(ctx, ICPMI_ERR_NULL, "out is NULL");
    if (ctx->comm || ctx->cb_allreduce)
        return fail(ctx, ICPMI_ERR_ARG, "a context with a communicator keeps no normal matrix (its sums are the ranks' shares)");
    if (k < 0 || k >= ctx->nm_count)
        return fail(ctx, ICPMI_ERR_ARG, "problem %d: the last registration call on this context ran %d", (int)k, ctx->nm_count);
    const icpmi_ctx *c = k == 0 ? ctx : ctx->helpers[(size_t)k - 1]->helper;
    if (!c->nm_valid)
        return fail(ctx, ICPMI_ERR_ARG, "no normal matrix: no registration ran, it failed, or its last pass kept no row");
    *out = c->nm;
    return ICPMI_OK;
}

int icpmi_nearest_batch(icpmi_ctx *ctx, const double *targets_xyz, int64_t n_tgt,
                        const double *queries_xyz, int64_t n_qry, int32_t *indices, double *dist_sq)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!targets_xyz || !queries_xyz || !indices) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (n_tgt <= 0) return fail(ctx, ICPMI_ERR_EMPTY_TARGET, "empty target cloud");
    if (n_qry < 0) return fail(ctx, ICPMI_ERR_ARG, "n_qry < 0");
    if (n_qry > (int64_t)700000000 || n_tgt > (int64_t)700000000) return fail(ctx, ICPMI_ERR_ARG, "cloud larger than 7e8 points");
    if (n_qry == 0) return ICPMI_OK;
    const int n = (int)n_qry, m = (int)n_tgt;
    if ((rc = reserve(ctx, ctx->stage_b, sizeof(double) * 3 * (size_t)n))) return rc;
    if ((rc = reserve(ctx, ctx->stage_c, sizeof(double) * 3 * (size_t)m))) return rc;
    ctx->loop_idx_valid = false; // (the search below writes its indices into idx)
    if ((rc = reserve(ctx, ctx->idx, sizeof(int) * (size_t)n))) return rc;
    if ((rc = reserve(ctx, ctx->d2out, sizeof(double) * (size_t)n))) return rc;
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_b.p, queries_xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_c.p, targets_xyz, sizeof(double) * 3 * (size_t)m, hipMemcpyHostToDevice, s));
    if ((rc = prepare_nn(ctx, (const double *)ctx->stage_c.p, m, n))) return rc;
    if ((rc = launch_nn(ctx, (const double *)ctx->stage_b.p, n, (const double *)ctx->stage_c.p, m,
                        (int *)ctx->idx.p, (double *)ctx->d2out.p, nullptr)))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(indices, ctx->idx.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
    if (dist_sq)
        HIP_TRY(ctx, hipMemcpyAsync(dist_sq, ctx->d2out.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    harvest_profile(ctx);
    return ICPMI_OK;
}

int icpmi_estimate_normals(icpmi_ctx *ctx, const double *points_xyz, int64_t n, int32_t k,
                           double *normals_xyz)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!points_xyz || !normals_xyz) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (n <= 0) return fail(ctx, ICPMI_ERR_EMPTY_TARGET, "empty cloud");
    if (n > (int64_t)700000000) return fail(ctx, ICPMI_ERR_ARG, "cloud larger than 7e8 points");
    if (k < 1 || k > 64) return fail(ctx, ICPMI_ERR_ARG, "k %d outside [1,64]", k);
    const int m = (int)n;
    if ((rc = reserve(ctx, ctx->stage_c, sizeof(double) * 3 * (size_t)m))) return rc;
    if ((rc = reserve(ctx, ctx->tgt.nrm, sizeof(double) * 3 * (size_t)m))) return rc;
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_c.p, points_xyz, sizeof(double) * 3 * (size_t)m, hipMemcpyHostToDevice, s));
    if ((rc = prepare_nn(ctx, (const double *)ctx->stage_c.p, m, m))) return rc;
    const bool sorted_rows = sorted_normal_rows(ctx, k, m);
    if ((rc = launch_normals(ctx, (const double *)ctx->stage_c.p, m, k, 0, m, (double *)ctx->tgt.nrm.p, sorted_rows, true))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(normals_xyz, ctx->tgt.nrm.p, sizeof(double) * 3 * (size_t)m, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    harvest_profile(ctx);
    return ICPMI_OK;
}

int icpmi_k_nearest(icpmi_ctx *ctx, const double *targets_xyz, int64_t n_tgt, const double *queries_xyz,
                    int64_t n_qry, int32_t k, int32_t *indices, double *dist_sq)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!targets_xyz || !queries_xyz || !indices) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (n_tgt <= 0) return fail(ctx, ICPMI_ERR_EMPTY_TARGET, "empty target cloud");
    if (n_qry < 0) return fail(ctx, ICPMI_ERR_ARG, "n_qry < 0");
    if (k < 1 || k > 64) return fail(ctx, ICPMI_ERR_ARG, "k %d outside [1,64]", k);
    if (n_qry > (int64_t)30000000 || n_tgt > (int64_t)700000000) return fail(ctx, ICPMI_ERR_ARG, "cloud too large");
    if (n_qry == 0) return ICPMI_OK;
    const int n = (int)n_qry, m = (int)n_tgt;
    if ((rc = reserve(ctx, ctx->stage_b, sizeof(double) * 3 * (size_t)n))) return rc;
    if ((rc = reserve(ctx, ctx->stage_c, sizeof(double) * 3 * (size_t)m))) return rc;
    if ((rc = reserve(ctx, ctx->knn_idx, sizeof(int) * (size_t)std::max(m, n) * k))) return rc;
    if (dist_sq && (rc = reserve(ctx, ctx->d2out, sizeof(double) * (size_t)n * k))) return rc;
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_b.p, queries_xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_c.p, targets_xyz, sizeof(double) * 3 * (size_t)m, hipMemcpyHostToDevice, s));
    // entries a list does not reach (k > n_tgt, a query with a NaN coordinate) stay -1 / +infinity
    HIP_TRY(ctx, hipMemsetAsync(ctx->knn_idx.p, 0xFF, sizeof(int) * (size_t)n * k, s));
    if ((rc = prepare_nn(ctx, (const double *)ctx->stage_c.p, m, n))) return rc;
    if ((rc = launch_knn(ctx, (const double *)ctx->stage_b.p, n, (const double *)ctx->stage_c.p, m, k, 0, n))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(indices, ctx->knn_idx.p, sizeof(int) * (size_t)n * k, hipMemcpyDeviceToHost, s));
    if (dist_sq) {
        for (size_t e = 0; e < (size_t)n * k; ++e) dist_sq[e] = __builtin_inf();
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d2out.p, dist_sq, sizeof(double) * (size_t)n * k, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_knn_distances, dim3((unsigned)(((size_t)n * k + 255) / 256)), dim3(256), 0, s,
                           (const double *)ctx->stage_b.p, n, (const double *)ctx->stage_c.p, m, k,
                           (const int *)ctx->knn_idx.p, (double *)ctx->d2out.p);
        HIP_TRY(ctx, hipMemcpyAsync(dist_sq, ctx->d2out.p, sizeof(double) * (size_t)n * k, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipGetLastError());
    harvest_profile(ctx);
    return ICPMI_OK;
}

int icpmi_solve_point_to_plane(icpmi_ctx *ctx, const double *source_xyz, const double *target_xyz,
                               const double *normals_xyz, int64_t n64, double transform_out[16])
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!source_xyz || !target_xyz || !normals_xyz || !transform_out)
        return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (n64 <= 0) return fail(ctx, ICPMI_ERR_EMPTY_SOURCE, "empty correspondence set");
    if (n64 > (int64_t)700000000) return fail(ctx, ICPMI_ERR_ARG, "more than 7e8 correspondences");
    const int n = (int)n64;
    const size_t bytes = sizeof(double) * 3 * (size_t)n;
    if ((rc = reserve(ctx, ctx->stage_a, bytes))) return rc;
    if ((rc = reserve(ctx, ctx->stage_b, bytes))) return rc;
    if ((rc = reserve(ctx, ctx->stage_c, bytes))) return rc;
    const int rblocks = reduce_blocks(ctx->cu_count, n);
    if ((rc = reserve(ctx, ctx->partials, sizeof(double) * kSumsStride * (size_t)rblocks))) return rc;
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_a.p, source_xyz, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_b.p, target_xyz, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_c.p, normals_xyz, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_state, 0, sizeof(IcpState), s));
    {
        StageTimer t(ctx, ST_REDUCE);
        hipLaunchKernelGGL(k_reduce_rule<RuleNone>, dim3(rblocks), dim3(256), 0, s, (const double *)ctx->stage_a.p, n,
                           (const double *)ctx->stage_b.p, n, (const double *)ctx->stage_c.p,
                           (const int *)nullptr, (double *)ctx->partials.p, (const IcpState *)nullptr);
        hipLaunchKernelGGL(k_finish_solve, dim3(1), dim3(kFinishThreads), 0, s, (const double *)ctx->partials.p,
                           rblocks, n, ctx->d_state);
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_state, ctx->d_state, sizeof(IcpState), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipGetLastError());
    harvest_profile(ctx);
    memcpy(transform_out, ctx->h_state->delta, sizeof(double) * 16);
    return ICPMI_OK;
}

int icpmi_transform_points(icpmi_ctx *ctx, const double transform[16], const double *in_xyz,
                           int64_t n64, double *out_xyz)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!transform || !in_xyz || !out_xyz) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (n64 < 0 || n64 > (int64_t)700000000) return fail(ctx, ICPMI_ERR_ARG, "n out of range");
    if (n64 == 0) return ICPMI_OK;
    const int n = (int)n64;
    const size_t bytes = sizeof(double) * 3 * (size_t)n;
    if ((rc = reserve(ctx, ctx->stage_a, bytes))) return rc;
    hipStream_t s = ctx->stream;
    memset(ctx->h_state, 0, sizeof(IcpState));
    memcpy(ctx->h_state->total, transform, sizeof(double) * 16);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_state, ctx->h_state, sizeof(IcpState), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_a.p, in_xyz, bytes, hipMemcpyHostToDevice, s));
    {
        StageTimer t(ctx, ST_TRANSFORM);
        hipLaunchKernelGGL(k_transform, dim3(std::min(2048, (n + 255) / 256)), dim3(256), 0, s,
                           (const double *)ctx->stage_a.p, (double *)ctx->stage_a.p, n, ctx->d_state, 1, 0);
    }
    HIP_TRY(ctx, hipMemcpyAsync(out_xyz, ctx->stage_a.p, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipGetLastError());
    harvest_profile(ctx);
    return ICPMI_OK;
}

int icpmi_voxel_downsample_device(icpmi_ctx *ctx, const double *d_points_xyz, int64_t n, double voxel_size,
                                  double *d_out_xyz, int64_t out_cap, int64_t *n_out)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!d_points_xyz || !d_out_xyz || !n_out) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (n < 0 || n > 700000000) return fail(ctx, ICPMI_ERR_ARG, "n out of range");
    *n_out = 0;
    if (n == 0) return ICPMI_OK;
    return voxel_downsample_device(ctx, d_points_xyz, (int)n, voxel_size, d_out_xyz, out_cap, n_out);
}

int icpmi_voxel_downsample(icpmi_ctx *ctx, const double *points_xyz, int64_t n, double voxel_size,
                           double *out_xyz, int64_t out_cap, int64_t *n_out)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!points_xyz || !out_xyz || !n_out) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (n < 0 || n > 700000000) return fail(ctx, ICPMI_ERR_ARG, "n out of range");
    *n_out = 0;
    if (n == 0) return ICPMI_OK;
    const size_t bytes = sizeof(double) * 3 * (size_t)n;
    if ((rc = reserve(ctx, ctx->stage_a, bytes))) return rc;
    if ((rc = reserve(ctx, ctx->vox_out, bytes))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_a.p, points_xyz, bytes, hipMemcpyHostToDevice, ctx->stream));
    int64_t rows = 0;
    if ((rc = voxel_downsample_device(ctx, (const double *)ctx->stage_a.p, (int)n, voxel_size,
                                      (double *)ctx->vox_out.p, n, &rows)))
        return rc;
    if (rows > out_cap) return fail(ctx, ICPMI_ERR_CAPACITY, "output holds %lld rows, needs %lld", (long long)out_cap, (long long)rows);
    HIP_TRY(ctx, hipMemcpy(out_xyz, ctx->vox_out.p, sizeof(double) * 3 * (size_t)rows, hipMemcpyDeviceToHost));
    *n_out = rows;
    return ICPMI_OK;
}

// ---- on-disk formats: host-side, no device work ------------------
// KITTI .bin: x, y, z, intensity as float32, intensity dropped (file_utils.cpp:115-141).
// PLY: header parse as file_utils.cpp:31-60 (every `property` line counts towards the vertex
// stride, whatever element it belongs to -- like the reference); binary payload read as
// little-endian float32 at the x/y/z offsets whatever the declared type or endianness
// (file_utils.cpp:87-98); ASCII payload: first three numbers of each line (file_utils.cpp:100-104).
int icpmi_load_cloud(const char *path, double *out_xyz, int64_t cap, int64_t *n_out)
{
    if (!path || !n_out) return fail(nullptr, ICPMI_ERR_NULL, "null argument");
    *n_out = 0;
    FILE *f = fopen(path, "rb");
    if (!f) return fail(nullptr, ICPMI_ERR_ARG, "Cannot open file: %s", path); // file_utils.cpp:22-24
    struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
    const size_t len = strlen(path);
    if (len >= 4 && strcmp(path + len - 4, ".bin") == 0) {
        fseek(f, 0, SEEK_END);
        const long size = ftell(f);
        fseek(f, 0, SEEK_SET);
        const int64_t n = size / (4 * (long)sizeof(float)); // file_utils.cpp:127
        *n_out = n;
        if (!out_xyz) return ICPMI_OK;
        if (cap < n) return fail(nullptr, ICPMI_ERR_CAPACITY, "output holds %lld rows, needs %lld", (long long)cap, (long long)n);
        std::vector<float> buf(4 * 4096);
        for (int64_t i = 0; i < n;) {
            const size_t want = (size_t)std::min<int64_t>(4096, n - i);
            const size_t got = fread(buf.data(), 4 * sizeof(float), want, f);
            for (size_t k = 0; k < got; ++k)
                for (int a = 0; a < 3; ++a) out_xyz[3 * (i + k) + a] = (double)buf[4 * k + a];
            for (size_t k = got; k < want; ++k)
                for (int a = 0; a < 3; ++a) out_xyz[3 * (i + k) + a] = 0.0;
            i += want;
        }
        return ICPMI_OK;
    }
    // PLY header
    std::string line;
    auto getline = [&](std::string &s) -> bool {
        s.clear();
        int ch;
        while ((ch = fgetc(f)) != EOF) {
            if (ch == '\n') return true;
            s.push_back((char)ch);
        }
        return !s.empty();
    };
    long num_vertices = 0;
    bool is_binary = false;
    std::vector<std::pair<std::string, std::string>> props;
    while (getline(line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back(); // file_utils.cpp:34-36
        char tok[64] = "", a[64] = "", b[64] = "";
        const int nt = sscanf(line.c_str(), "%63s %63s %63s", tok, a, b);
        if (nt < 1) continue;
        if (!strcmp(tok, "format")) {
            if (!strcmp(a, "binary_little_endian") || !strcmp(a, "binary_big_endian")) is_binary = true;
        } else if (!strcmp(tok, "element")) {
            if (!strcmp(a, "vertex")) num_vertices = nt >= 3 ? atol(b) : 0;
        } else if (!strcmp(tok, "property")) {
            props.emplace_back(std::string(b), std::string(a)); // (name, dtype), file_utils.cpp:54-56
        } else if (!strcmp(tok, "end_header")) {
            break;
        }
    }
    auto type_size = [](const std::string &t) -> size_t { // file_utils.cpp:63-70
        if (t == "float" || t == "float32") return 4;
        if (t == "double" || t == "float64") return 8;
        if (t == "uchar" || t == "uint8" || t == "char" || t == "int8") return 1;
        if (t == "ushort" || t == "uint16" || t == "short" || t == "int16") return 2;
        if (t == "uint" || t == "uint32" || t == "int" || t == "int32") return 4;
        return 4;
    };
    size_t stride = 0, xo = 0, yo = 0, zo = 0;
    for (auto &pr : props) {
        if (pr.first == "x") xo = stride;
        else if (pr.first == "y") yo = stride;
        else if (pr.first == "z") zo = stride;
        stride += type_size(pr.second);
    }
    const int64_t n = num_vertices > 0 ? num_vertices : 0;
    *n_out = n;
    if (!out_xyz) return ICPMI_OK;
    if (cap < n) return fail(nullptr, ICPMI_ERR_CAPACITY, "output holds %lld rows, needs %lld", (long long)cap, (long long)n);
    if (is_binary) {
        if (stride < 4 || xo + 4 > stride || yo + 4 > stride || zo + 4 > stride)
            return fail(nullptr, ICPMI_ERR_ARG, "PLY vertex layout has no float x/y/z");
        std::vector<char> buf(stride);
        for (int64_t i = 0; i < n; ++i) {
            if (fread(buf.data(), 1, stride, f) != stride) memset(buf.data(), 0, stride);
            float v[3];
            memcpy(&v[0], buf.data() + xo, 4);
            memcpy(&v[1], buf.data() + yo, 4);
            memcpy(&v[2], buf.data() + zo, 4);
            for (int a2 = 0; a2 < 3; ++a2) out_xyz[3 * i + a2] = (double)v[a2];
        }
    } else {
        for (int64_t i = 0; i < n; ++i) {
            double v[3] = {0, 0, 0};
            if (getline(line)) sscanf(line.c_str(), "%lf %lf %lf", &v[0], &v[1], &v[2]);
            for (int a2 = 0; a2 < 3; ++a2) out_xyz[3 * i + a2] = v[a2];
        }
    }
    return ICPMI_OK;
}

// ---- frame files of a sequence directory (file_utils.cpp:203-247) ---------------------------------
// The reference's std::regex_search(filename, "(\\d+)\\.ply") finds the leftmost run of digits that is
// followed by the extension: a run followed by anything else can only fail (the greedy \d+ has
// nothing to give back that "\\." would match), so no regex engine is needed.
static bool frame_number(const char *name, const char *ext, long long *out)
{
    const size_t el = strlen(ext);
    for (size_t i = 0; name[i];) {
        if (name[i] < '0' || name[i] > '9') {
            ++i;
            continue;
        }
        size_t j = i;
        while (name[j] >= '0' && name[j] <= '9') ++j;
        if (strncmp(name + j, ext, el) == 0) {
            if (j - i > 18) return false; // std::stoll would throw std::out_of_range: not a frame
            long long v = 0;
            for (size_t k = i; k < j; ++k) v = v * 10 + (name[k] - '0');
            *out = v;
            return true;
        }
        i = j;
    }
    return false;
}

int icpmi_discover_frames(const char *data_dir, int64_t *stamps, int64_t frames_cap, char *paths, int64_t paths_cap,
                          int64_t *n_frames, int64_t *paths_bytes)
{
    if (!data_dir || !n_frames || !paths_bytes) return fail(nullptr, ICPMI_ERR_NULL, "null argument");
    *n_frames = 0;
    *paths_bytes = 0;
    if (!*data_dir) return fail(nullptr, ICPMI_ERR_ARG, "empty directory name");
    DIR *d = opendir(data_dir);
    if (!d) return fail(nullptr, ICPMI_ERR_ARG, "Cannot open directory: %s", data_dir); // fs::directory_iterator throws
    std::vector<std::pair<long long, std::string>> frames;
    while (struct dirent *e = readdir(d)) {
        const char *name = e->d_name;
        const char *dot = strrchr(name, '.');
        if (!dot || dot == name) continue; // path::extension() of ".ply" / "x" is empty
        long long stamp = -1;
        // file_utils.cpp:224-241: extension first, then the number in front of that extension's first occurrence
        if ((strcmp(dot, ".ply") == 0 && frame_number(name, ".ply", &stamp)) ||
            (strcmp(dot, ".bin") == 0 && frame_number(name, ".bin", &stamp)))
            frames.emplace_back(stamp, std::string(data_dir) + (data_dir[strlen(data_dir) - 1] == '/' ? "" : "/") + name);
    }
    closedir(d);
    // file_utils.cpp:244-245 sorts by number only (std::sort: equal numbers in unspecified order);
    // here equal numbers come out by path so that the result does not depend on the file system
    std::sort(frames.begin(), frames.end());
    int64_t bytes = 0;
    for (auto &f : frames) bytes += (int64_t)f.second.size() + 1;
    *n_frames = (int64_t)frames.size();
    *paths_bytes = bytes;
    if (!stamps && !paths) return ICPMI_OK; // sizing call
    if (frames_cap < *n_frames || paths_cap < bytes)
        return fail(nullptr, ICPMI_ERR_CAPACITY, "%lld frames / %lld path bytes do not fit", (long long)*n_frames, (long long)bytes);
    char *w = paths;
    for (size_t i = 0; i < frames.size(); ++i) {
        if (stamps) stamps[i] = frames[i].first;
        if (paths) {
            memcpy(w, frames[i].second.c_str(), frames[i].second.size() + 1);
            w += frames[i].second.size() + 1;
        }
    }
    return ICPMI_OK;
}

int icpmi_upload_points_f32(icpmi_ctx *ctx, const float *records, int64_t n, int32_t stride_floats, double *d_out_xyz)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!records || !d_out_xyz) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (n < 0 || n > 700000000) return fail(ctx, ICPMI_ERR_ARG, "n out of range");
    if (stride_floats < 3 || stride_floats > 64) return fail(ctx, ICPMI_ERR_ARG, "stride %d outside [3,64]", stride_floats);
    if (n == 0) return ICPMI_OK;
    const size_t bytes = sizeof(float) * (size_t)stride_floats * (size_t)n;
    if ((rc = reserve(ctx, ctx->f32_stage, bytes))) return rc;
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->f32_stage.p, records, bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_widen_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float *)ctx->f32_stage.p, (int)n,
                       (int)stride_floats, d_out_xyz);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return ICPMI_OK;
}

int icpmi_load_cloud_device(icpmi_ctx *ctx, const char *path, double *d_out_xyz, int64_t cap, int64_t *n_out)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!path || !n_out) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    *n_out = 0;
    const size_t len = strlen(path);
    if (len >= 4 && strcmp(path + len - 4, ".bin") == 0) {
        FILE *f = fopen(path, "rb");
        if (!f) return fail(ctx, ICPMI_ERR_ARG, "Cannot open file: %s", path); // file_utils.cpp:116-118
        struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
        fseek(f, 0, SEEK_END);
        const long size = ftell(f);
        fseek(f, 0, SEEK_SET);
        const int64_t n = size / (4 * (long)sizeof(float)); // file_utils.cpp:127
        *n_out = n;
        if (!d_out_xyz) return ICPMI_OK;
        if (cap < n) return fail(ctx, ICPMI_ERR_CAPACITY, "output holds %lld rows, needs %lld", (long long)cap, (long long)n);
        if (n == 0) return ICPMI_OK;
        std::vector<float> rec(4 * (size_t)n, 0.f); // (a short read leaves zeros, like the host loader)
        if (fread(rec.data(), 4 * sizeof(float), (size_t)n, f) != (size_t)n) { /* zeros stay */ }
        return icpmi_upload_points_f32(ctx, rec.data(), n, 4, d_out_xyz);
    }
    // PLY: header rules and the ASCII payload are host work (icpmi_load_cloud); fp64 rows go up as they are
    int64_t n = 0;
    if ((rc = icpmi_load_cloud(path, nullptr, 0, &n))) return fail(ctx, rc, "%s", icpmi_last_error(nullptr));
    *n_out = n;
    if (!d_out_xyz) return ICPMI_OK;
    if (cap < n) return fail(ctx, ICPMI_ERR_CAPACITY, "output holds %lld rows, needs %lld", (long long)cap, (long long)n);
    if (n == 0) return ICPMI_OK;
    std::vector<double> host(3 * (size_t)n);
    if ((rc = icpmi_load_cloud(path, host.data(), n, &n))) return fail(ctx, rc, "%s", icpmi_last_error(nullptr));
    HIP_TRY(ctx, hipMemcpy(d_out_xyz, host.data(), sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));
    return ICPMI_OK;
}

int icpmi_estimate_normals_rows(icpmi_ctx *ctx, const double *points_xyz, int64_t n, int32_t k, int64_t row0,
                                int64_t row1, double *normals_xyz)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!points_xyz || !normals_xyz) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (n <= 0) return fail(ctx, ICPMI_ERR_EMPTY_TARGET, "empty cloud");
    if (n > (int64_t)700000000) return fail(ctx, ICPMI_ERR_ARG, "cloud larger than 7e8 points");
    if (k < 1 || k > 64) return fail(ctx, ICPMI_ERR_ARG, "k %d outside [1,64]", k);
    if (row0 < 0 || row1 < row0 || row1 > n) return fail(ctx, ICPMI_ERR_ARG, "rows [%lld,%lld) outside [0,%lld)", (long long)row0, (long long)row1, (long long)n);
    if (row1 == row0) return ICPMI_OK;
    const int m = (int)n, rows = (int)(row1 - row0);
    if ((rc = reserve(ctx, ctx->stage_c, sizeof(double) * 3 * (size_t)m))) return rc;
    if ((rc = reserve(ctx, ctx->tgt.nrm, sizeof(double) * 3 * (size_t)m))) return rc;
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_c.p, points_xyz, sizeof(double) * 3 * (size_t)m, hipMemcpyHostToDevice, s));
    // a slice is always taken in point order (what a rank of a caller-sharded job wants back)
    const bool keep_pruned = ctx->tgt.nn_pruned;
    if ((rc = prepare_nn(ctx, (const double *)ctx->stage_c.p, m, m))) return rc;
    ctx->tgt.nn_pruned = false;
    rc = launch_normals(ctx, (const double *)ctx->stage_c.p, m, k, (int)row0, (int)row1, (double *)ctx->tgt.nrm.p, false, true);
    ctx->tgt.nn_pruned = keep_pruned;
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(normals_xyz, (const double *)ctx->tgt.nrm.p + 3 * (size_t)row0, sizeof(double) * 3 * (size_t)rows,
                                hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    harvest_profile(ctx);
    return ICPMI_OK;
}

// ---- odometry stream: the registration part of SlamNode::process_frame (slam_node.cpp:122-152) ---------
int icpmi_stream_reset(icpmi_ctx *ctx)
{
    if (!ctx) return ICPMI_ERR_NULL;
    ctx->stream_prev_n = -1;
    ctx->tgt.prep_valid = false;
    if (ctx->prep_helper) ctx->prep_helper->tgt.prep_valid = false; // (a preparation still in flight is waited for by the next push)
    return ICPMI_OK;
}

namespace {
int stream_check_args(icpmi_ctx *ctx, const icpmi_config *cfg, icpmi_result *result, double *error_history, int32_t history_cap,
                      icpmi_stream_info *info)
{
    if (!cfg || !result || !error_history || !info) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (cfg->max_iterations < 0) return fail(ctx, ICPMI_ERR_ARG, "max_iterations < 0");
    if (history_cap < cfg->max_iterations + 1)
        return fail(ctx, ICPMI_ERR_CAPACITY, "error_history holds %d entries, needs %d", history_cap, cfg->max_iterations + 1);
    memset(result, 0, sizeof(*result));
    for (int i = 0; i < 16; ++i) result->transformation[i] = (i % 5 == 0) ? 1.0 : 0.0;
    memset(info, 0, sizeof(*info));
    return ICPMI_OK;
}
int stream_register(icpmi_ctx *ctx, int64_t n_cur, int64_t min_points, const icpmi_config *cfg, icpmi_result *result,
                    double *error_history, int32_t history_cap, icpmi_stream_info *info);
int deskew_check_config(icpmi_ctx *ctx, const icpmi_deskew_config *cfg);
int deskew_queue(icpmi_ctx *ctx, const icpmi_deskew_config *cfg, const double *d_xyz, const double *d_times, int64_t n, double *d_out);
} // namespace

int icpmi_stream_push(icpmi_ctx *ctx, const double *d_raw_xyz, int64_t n_raw, double voxel_size, int64_t min_points,
                      const icpmi_config *cfg, icpmi_result *result, double *error_history, int32_t history_cap,
                      icpmi_stream_info *info)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!d_raw_xyz) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (n_raw <= 0 || n_raw > 700000000) return fail(ctx, ICPMI_ERR_ARG, "n_raw out of range");
    if ((rc = stream_check_args(ctx, cfg, result, error_history, history_cap, info))) return rc;
    if (ctx->prefetch) { // what the worker filters the next file with
        std::lock_guard<std::mutex> lk(ctx->prefetch->mu);
        ctx->prefetch->voxel_hint = voxel_size;
    }
    if (ctx->stream_deskew_on) {
        // the raw scan into the frame of the sweep's t_ref first (deskew.h), queued in front of the filter: no wait
        if ((rc = deskew_check_config(ctx, &ctx->stream_deskew))) return rc;
        if ((rc = reserve(ctx, ctx->deskew_raw, sizeof(double) * 3 * (size_t)n_raw))) return rc;
        if ((rc = deskew_queue(ctx, &ctx->stream_deskew, d_raw_xyz, nullptr, n_raw, (double *)ctx->deskew_raw.p))) return rc;
        d_raw_xyz = (const double *)ctx->deskew_raw.p;
    }
    // curr = voxel_downsample(raw)  (slam_node.cpp:122), into the buffer that is not the previous frame
    if ((rc = reserve(ctx, ctx->stream_cur, sizeof(double) * 3 * (size_t)n_raw))) return rc;
    int64_t n_cur = 0;
    if ((rc = voxel_downsample_device(ctx, d_raw_xyz, (int)n_raw, voxel_size, (double *)ctx->stream_cur.p, n_raw, &n_cur, false))) return rc;
    return stream_register(ctx, n_cur, min_points, cfg, result, error_history, history_cap, info);
}

namespace {
// everything of a push behind the filter: ctx->stream_cur holds the n_cur rows of the filtered scan
int stream_register(icpmi_ctx *ctx, int64_t n_cur, int64_t min_points, const icpmi_config *cfg, icpmi_result *result,
                    double *error_history, int32_t history_cap, icpmi_stream_info *info)
{
    int rc;
    info->n_filtered = n_cur;
    info->n_target = ctx->stream_prev_n < 0 ? 0 : ctx->stream_prev_n;
    ctx->nm_valid = false; // (a push that registers nothing leaves no normal matrix)
    ctx->nm_count = 1;
    ctx->stream_robust_info = icpmi_robust_info{};
    GateRun rule{};
    if (ctx->stream_robust_on && (rc = validate_robust(ctx, &ctx->stream_robust, &rule))) return rc; // (a communicator set since)
    ctx->stream_cur_n = n_cur;
    // The scan just filtered is the NEXT push's target (slam_node.cpp:128,152): its search structure and
    // normals (Morton sort, split frames, operand packing, 20-NN, PCA: ~135 us of small kernels) are built on a
    // helper context -- a stream and workspace of their own -- BESIDE this push's registration, queued once the
    // registration's first iterations are (the host's launch time for them then hides behind the device's
    // work), and the next push adopts them by swapping buffers behind an event: this context's stream carries the
    // registration only.  (Round 2 queued the preparation on this stream behind the result: registration and
    // preparation in a row were the 0.31 ms of a frame.)
    const bool early = ctx->opt.profile == 0 && !(ctx->comm != nullptr || ctx->cb_allreduce != nullptr);
    if (early && !ctx->prep_helper) {
        icpmi_options o = ctx->opt;
        icpmi_ctx *h = nullptr;
        if (icpmi_create(&o, &h) == ICPMI_OK) ctx->prep_helper = h;
        if (ctx->prep_helper && !ctx->prep_done) (void)hipEventCreateWithFlags(&ctx->prep_done, hipEventDisableTiming);
        if (ctx->prep_helper && !ctx->scan_ready) (void)hipEventCreateWithFlags(&ctx->scan_ready, hipEventDisableTiming);
    }
    icpmi_ctx *helper = early && ctx->prep_done && ctx->scan_ready ? ctx->prep_helper : nullptr;
    // everything that produced the scan on this context's stream is queued by now: the helper's stream waits for it
    if (helper && n_cur > 0) HIP_TRY(ctx, hipEventRecord(ctx->scan_ready, ctx->stream));
    auto prepare_next = [](icpmi_ctx *c) -> int {
        icpmi_ctx *h = c->prep_helper;
        if (!h || c->stream_cur_n <= 0) return ICPMI_OK;
        struct Clock { icpmi_ctx *c; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
                       ~Clock() { c->t_prep_queue += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); } } clock{c};
        if (hipStreamWaitEvent(h->stream, c->scan_ready, 0) != hipSuccess) return ICPMI_ERR_HIP;
        const int r = prepare_target(h, (const double *)c->stream_cur.p, (int)c->stream_cur_n, (int)c->stream_cur_n);
        c->helper_busy = true; // (whatever was queued reads the scan: somebody has to wait for it before the scan's buffer is reused)
        if (r != ICPMI_OK || hipEventRecord(c->prep_done, h->stream) != hipSuccess) {
            h->tgt.prep_valid = false;
            (void)hipStreamSynchronize(h->stream);
            c->helper_busy = false;
            return ICPMI_ERR_HIP;
        }
        return ICPMI_OK;
    };
    // the target of THIS registration: prepared by the helper during the previous push?  Adopt it.
    if (helper && helper->tgt.prep_valid && ctx->stream_prev_n > 0 && helper->tgt.prep_tgt == (const double *)ctx->stream_prev.p &&
        helper->tgt.prep_m == (int)ctx->stream_prev_n) {
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->prep_done, 0));
        adopt_target(ctx, helper);
        ctx->helper_busy = false; // (this push's registration runs behind it, and the push waits for the registration)
    } else if (ctx->helper_busy) {
        // a preparation nobody is going to use (another scan was pushed in between, a stream reset): it still reads a
        // scan buffer of this stream -- wait for it before anything is queued that could write there
        HIP_TRY(ctx, hipEventSynchronize(ctx->prep_done));
        ctx->helper_busy = false;
        if (helper) helper->tgt.prep_valid = false;
    }
    bool queued_next = false;
    if (ctx->stream_prev_n < 0) {
        info->status = ICPMI_STREAM_FIRST_FRAME;          // slam_node.cpp:69-72: nothing to register against yet
    } else if (n_cur < min_points || n_cur <= 0 || ctx->stream_prev_n <= 0) { // (an empty cloud on either side is UB in the reference)
        info->status = ICPMI_STREAM_TOO_FEW_POINTS;       // slam_node.cpp:125-130: the caller repeats its last pose
    } else {
        // source = curr, target = prev (slam_node.cpp:132-133): both already in HBM; the target's
        // search structure and normals are the adopted ones (prepared during the previous push, as a rule)
        info->status = ICPMI_STREAM_REGISTERED;
        queued_next = helper != nullptr;
        static const bool span = getenv("ICPMI_STREAM_STATS") != nullptr;
        static hipEvent_t e0 = nullptr, e1 = nullptr;
        if (span && !e0) { (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); }
        if (span) (void)hipEventRecord(e0, ctx->stream);
        const auto ta = std::chrono::steady_clock::now();
        rc = align_device(ctx, (const double *)ctx->stream_cur.p, n_cur, (const double *)ctx->stream_prev.p,
                          ctx->stream_prev_n, cfg, result, error_history, history_cap, nullptr,
                          helper ? +prepare_next : nullptr, ctx->stream_robust_on ? &rule : nullptr);
        if (rc == ICPMI_OK && ctx->stream_robust_on) ctx->stream_robust_info = icpmi_robust_info{rule.weight_sum, rule.pairs, n_cur};
        ctx->t_align += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta).count();
        if (span) {
            (void)hipEventRecord(e1, ctx->stream);
            (void)hipEventSynchronize(e1);
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ctx->t_gpu_span += ms;
        }
        if (rc) {
            //  after_first may have queued the preparation of stream_cur on the helper: the buffers are not
            // swapped on this path, so the NEXT push filters into stream_cur again -- not under the helper's reads
            if (ctx->helper_busy) {
                (void)hipEventSynchronize(ctx->prep_done);
                ctx->helper_busy = false;
                if (helper) helper->tgt.prep_valid = false;
            }
            return rc;
        }
    }
    if (!queued_next && helper) (void)prepare_next(ctx); // (a failure only means the next push prepares its target itself)
    std::swap(ctx->stream_prev, ctx->stream_cur);         // prev_points_ = curr (slam_node.cpp:128,152), no copy
    ctx->stream_prev_n = n_cur;
    return ICPMI_OK;
}
} // namespace

int icpmi_stream_set_robust(icpmi_ctx *ctx, const icpmi_robust *rule)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!rule) {
        ctx->stream_robust_on = false;
        return ICPMI_OK;
    }
    GateRun run;
    if ((rc = validate_robust(ctx, rule, &run))) return rc;
    ctx->stream_robust = *rule;
    ctx->stream_robust_on = true;
    return ICPMI_OK;
}

int icpmi_stream_last_robust(icpmi_ctx *ctx, icpmi_robust_info *info)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!info) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    *info = ctx->stream_robust_info;
    return ICPMI_OK;
}

namespace {
bool is_bin(const char *path)
{
    const size_t len = strlen(path);
    return len >= 4 && strcmp(path + len - 4, ".bin") == 0;
}
void prefetch_worker(FilePrefetch *pf)
{
    (void)hipSetDevice(pf->device);
    std::unique_lock<std::mutex> lk(pf->mu);
    for (;;) {
        pf->cv.wait(lk, [pf] { return pf->quit || pf->busy; });
        if (pf->quit) return;
        const std::string path = pf->want;
        // the slot to fill: an empty one, else the older of two files that were prefetched but never pushed.  A push
        // may have read the slot: its kernels are behind the event it recorded (another stream than this thread's)
        const int slot = pf->taking >= 0 ? 1 - pf->taking
                                         : (pf->ready[0].empty() ? 0 : (pf->ready[1].empty() ? 1 : (pf->ready_seq[0] < pf->ready_seq[1] ? 0 : 1)));
        pf->ready[slot].clear();
        const bool wait_for_push = pf->slot_used[slot];
        const double voxel = pf->voxel_hint;
        lk.unlock();
        auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        const double ta = now();
        if (wait_for_push) (void)hipEventSynchronize(pf->slot_done[slot]);
        const double tb = now();
        double tc = tb, td = tb, te = tb;
        bool ok = false;
        int64_t n = 0;
        if (FILE *f = fopen(path.c_str(), "rb")) {
            fseek(f, 0, SEEK_END);
            const long size = ftell(f);
            fseek(f, 0, SEEK_SET);
            n = size / (4 * (long)sizeof(float)); // file_utils.cpp:127
            if (n > 0 && n <= 700000000) {
                const size_t bytes = 4 * sizeof(float) * (size_t)n;
                if (pf->h_cap[slot] < bytes) {
                    // (the copies out of this slot's staging buffer finished long ago: the slot's previous file has been pushed)
                    if (pf->h_buf[slot]) (void)hipHostFree(pf->h_buf[slot]);
                    pf->h_buf[slot] = nullptr;
                    pf->h_cap[slot] = 0;
                    if (hipHostMalloc(&pf->h_buf[slot], bytes + bytes / 4, hipHostMallocDefault) == hipSuccess) pf->h_cap[slot] = bytes + bytes / 4;
                }
                if (!pf->h_runs && hipHostMalloc((void **)&pf->h_runs, 4 * sizeof(unsigned), hipHostMallocDefault) != hipSuccess) pf->h_runs = nullptr;
                if (pf->d_cap[slot] < (size_t)n) {
                    if (pf->stream) (void)hipStreamSynchronize(pf->stream);
                    if (pf->d_f32[slot]) (void)hipFree(pf->d_f32[slot]);
                    if (pf->d_raw[slot]) (void)hipFree(pf->d_raw[slot]);
                    pf->d_f32[slot] = nullptr;
                    pf->d_raw[slot] = nullptr;
                    pf->d_cap[slot] = 0;
                    const size_t cap = (size_t)n + (size_t)n / 4;
                    if (hipMalloc(&pf->d_f32[slot], 4 * sizeof(float) * cap) == hipSuccess &&
                        hipMalloc((void **)&pf->d_raw[slot], 3 * sizeof(double) * cap) == hipSuccess)
                        pf->d_cap[slot] = cap;
                }
                if (!pf->stream) (void)hipStreamCreateWithFlags(&pf->stream, hipStreamNonBlocking);
                if (pf->stream && !pf->filled[slot]) (void)hipEventCreateWithFlags(&pf->filled[slot], hipEventDisableTiming);
                if (pf->h_cap[slot] >= bytes && pf->d_cap[slot] >= (size_t)n && pf->stream && pf->filled[slot] && pf->h_runs) {
                    // the file in two parts, the first one on its way to the device while the second is read; then the
                    // widening and the filter are queued behind the copies and an event behind them all: this thread
                    // waits for nothing of it
                    char *h = (char *)pf->h_buf[slot];
                    const size_t half = (bytes / 2) / 16 * 16;
                    const size_t got = fread(h, 1, half, f);
                    if (got < half) memset(h + got, 0, bytes - got); // a short read leaves zeros, like the synchronous path
                    bool up = hipMemcpyAsync(pf->d_f32[slot], h, half, hipMemcpyHostToDevice, pf->stream) == hipSuccess;
                    if (got == half) {
                        const size_t got2 = fread(h + half, 1, bytes - half, f);
                        if (got2 < bytes - half) memset(h + half + got2, 0, bytes - half - got2);
                    }
                    tc = now();
                    up = up && hipMemcpyAsync((char *)pf->d_f32[slot] + half, h + half, bytes - half, hipMemcpyHostToDevice, pf->stream) == hipSuccess;
                    if (up) {
                        hipLaunchKernelGGL(k_widen_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, pf->stream,
                                           (const float *)pf->d_f32[slot], (int)n, 4, pf->d_raw[slot]);
                        td = now();
                        pf->filtered_voxel[slot] = 0.0;
                        pf->pend_filtered[slot] = false;
                        if (voxel > 0.0 && reserve_raw(pf->filtered[slot], sizeof(double) * 3 * (size_t)n) == hipSuccess) {
                            const VoxelScratch vs{&pf->sc_bbox, &pf->sc_box, &pf->sc_keys, &pf->sc_vals, &pf->sc_tmp, 0};
                            const char *msg = "";
                            int64_t unused = 0;
                            pf->h_runs[2 * slot] = 0u;
                            pf->h_runs[2 * slot + 1] = 1u; // (reads as "could not be keyed" until the filter's own words arrive)
                            pf->pend_filtered[slot] = voxel_filter_core(pf->stream, vs, pf->d_raw[slot], (int)n, voxel, (double *)pf->filtered[slot].p, n,
                                                                        &unused, true, &msg, true, pf->h_runs + 2 * slot) == ICPMI_OK;
                            pf->pend_voxel[slot] = voxel;
                            // (a filter that could not be queued, or whose outcome says the grid cannot be keyed: the push
                            // filters the raw points itself and reports what is wrong with them)
                        }
                        ok = hipEventRecord(pf->filled[slot], pf->stream) == hipSuccess && hipGetLastError() == hipSuccess;
                    }
                }
            }
            fclose(f);
        }
        te = now();
        pf->t_wait += tb - ta, pf->t_read += tc - tb, pf->t_upload += td - tc, pf->t_filter += te - td, pf->files += 1;
        lk.lock();
        if (ok) {
            pf->ready[slot] = path;
            pf->ready_n[slot] = n;
            pf->ready_seq[slot] = ++pf->seq;
            pf->pending[slot] = true; // (the push waits for `filled[slot]`)
        }
        pf->want.clear();
        pf->busy = false;
        pf->cv.notify_all();
    }
}
} // namespace

int icpmi_stream_prefetch_file(icpmi_ctx *ctx, const char *path)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!path) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (ctx->stream_deskew_on)
        return fail(ctx, ICPMI_ERR_ARG, "icpmi_stream_prefetch_file with deskew set: the worker filters a file before its twist is known");
    if (!is_bin(path)) return ICPMI_OK; // a PLY goes through the host parser when it is pushed: nothing to do ahead
    if (!ctx->prefetch) {
        ctx->prefetch = new FilePrefetch();
        ctx->prefetch->device = ctx->opt.device;
        ctx->prefetch->worker = std::thread(prefetch_worker, ctx->prefetch);
    }
    FilePrefetch *pf = ctx->prefetch;
    {
        std::unique_lock<std::mutex> lk(pf->mu);
        if (pf->ready[0] == path || pf->ready[1] == path || (pf->busy && pf->want == path)) return ICPMI_OK; // already there / on its way
        pf->cv.wait(lk, [pf] { return !pf->busy; }); // one read at a time
        pf->want = path;
        pf->busy = true;
    }
    pf->cv.notify_all();
    return ICPMI_OK;
}

int icpmi_stream_push_file(icpmi_ctx *ctx, const char *path, double voxel_size, int64_t min_points, const icpmi_config *cfg,
                           icpmi_result *result, double *error_history, int32_t history_cap, icpmi_stream_info *info)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!path) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (ctx->stream_deskew_on)
        return fail(ctx, ICPMI_ERR_ARG, "icpmi_stream_push_file with deskew set: push the scan with icpmi_stream_push or icpmi_stream_push_host");
    struct PushClock { icpmi_ctx *c; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
                       ~PushClock() { c->t_push += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); c->pushes += 1; } } push_clock{ctx};
    if (!is_bin(path)) {
        // PLY: host parser (header rules, ASCII numbers), then the host-pointer form
        int64_t n = 0;
        if ((rc = icpmi_load_cloud(path, nullptr, 0, &n))) return fail(ctx, rc, "%s", icpmi_last_error(nullptr));
        if (n <= 0) return fail(ctx, ICPMI_ERR_ARG, "no points in %s", path);
        std::vector<double> host(3 * (size_t)n);
        if ((rc = icpmi_load_cloud(path, host.data(), n, &n))) return fail(ctx, rc, "%s", icpmi_last_error(nullptr));
        return icpmi_stream_push_host(ctx, host.data(), n, voxel_size, min_points, cfg, result, error_history, history_cap, info);
    }
    // KITTI .bin: the file is read into pinned memory and everything behind it -- copy, widening,
    // voxel filter, registration -- is queued on the context's stream without a wait in between
    if (FilePrefetch *pf = ctx->prefetch) { // already on the device (or on its way) thanks to the worker?
        std::unique_lock<std::mutex> lk(pf->mu);
        if (pf->busy && pf->want == path) pf->cv.wait(lk, [pf] { return !pf->busy; });
        const int slot = pf->ready[0] == path ? 0 : (pf->ready[1] == path ? 1 : -1);
        if (slot >= 0) {
            const int64_t n = pf->ready_n[slot];
            pf->taking = slot; // the worker fills the other one meanwhile
            lk.unlock();
            if (pf->pending[slot]) {
                // the worker announced the file with its copies, the widening and the filter still queued: wait for them here,
                // then look at what the filter left in pinned memory
                pf->pending[slot] = false;
                const auto tw = std::chrono::steady_clock::now();
                const bool arrived = hipEventSynchronize(pf->filled[slot]) == hipSuccess;
                ctx->t_wait_file += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw).count();
                if (arrived && pf->pend_filtered[slot] && pf->h_runs[2 * slot + 1] == 0u && (int64_t)pf->h_runs[2 * slot] <= n) {
                    pf->filtered_n[slot] = (int64_t)pf->h_runs[2 * slot];
                    pf->filtered_voxel[slot] = pf->pend_voxel[slot];
                }
                if (!arrived) { // the slot's contents cannot be trusted: the synchronous path below reads the file itself
                    (void)hipGetLastError();
                    lk.lock();
                    pf->ready[slot].clear();
                    pf->slot_used[slot] = false;
                    pf->taking = -1;
                    lk.unlock();
                    goto read_it_here;
                }
            }
            int rc2;
            if (pf->filtered_voxel[slot] > 0.0 && pf->filtered_voxel[slot] == voxel_size) {
                // the worker filtered it too: its buffer becomes the current scan (ours goes to the worker in exchange;
                // it holds the scan before the previous one, which nothing reads any more).  The arguments are
                // checked before anything is taken, and a registration that fails hands the buffer back: the
                // frame stays in its slot and a second push of the path finds it.
                if ((rc2 = stream_check_args(ctx, cfg, result, error_history, history_cap, info)) == ICPMI_OK) {
                    std::swap(ctx->stream_cur, pf->filtered[slot]);
                    rc2 = stream_register(ctx, pf->filtered_n[slot], min_points, cfg, result, error_history, history_cap, info);
                    if (rc2 != ICPMI_OK) std::swap(ctx->stream_cur, pf->filtered[slot]);
                }
                std::lock_guard<std::mutex> lk2(pf->mu);
                pf->voxel_hint = voxel_size;
            } else {
                rc2 = icpmi_stream_push(ctx, pf->d_raw[slot], n, voxel_size, min_points, cfg, result, error_history, history_cap, info);
            }
            if (!pf->slot_done[slot]) (void)hipEventCreateWithFlags(&pf->slot_done[slot], hipEventDisableTiming);
            const bool recorded = pf->slot_done[slot] && hipEventRecord(pf->slot_done[slot], ctx->stream) == hipSuccess;
            if (!recorded) (void)hipStreamSynchronize(ctx->stream); // (then the slot is simply free)
            lk.lock();
            pf->slot_used[slot] = recorded;
            if (rc2 == ICPMI_OK) pf->ready[slot].clear(); // free for the worker, behind the event (a failed push leaves the frame there)
            pf->taking = -1;
            lk.unlock();
            return rc2;
        }
        // not there (never asked for, or the worker could not read it): the synchronous path reads it and reports
    }
read_it_here:
    FILE *f = fopen(path, "rb");
    if (!f) return fail(ctx, ICPMI_ERR_ARG, "Cannot open file: %s", path); // file_utils.cpp:116-118
    struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    const int64_t n = size / (4 * (long)sizeof(float)); // file_utils.cpp:127
    if (n <= 0 || n > 700000000) return fail(ctx, ICPMI_ERR_ARG, "%lld points in %s", (long long)n, path);
    const size_t bytes = 4 * sizeof(float) * (size_t)n;
    if (ctx->h_file_cap < bytes) {
        if (ctx->h_file) (void)hipHostFree(ctx->h_file);
        ctx->h_file = nullptr;
        ctx->h_file_cap = 0;
        HIP_TRY(ctx, hipHostMalloc(&ctx->h_file, bytes + bytes / 4, hipHostMallocDefault));
        ctx->h_file_cap = bytes + bytes / 4;
    }
    // (the previous frame's copy out of this buffer finished long ago: every push ends with a stream wait)
    const size_t got = fread(ctx->h_file, 1, bytes, f);
    if (got < bytes) memset((char *)ctx->h_file + got, 0, bytes - got); // a short read leaves zeros, like the host loader
    if ((rc = reserve(ctx, ctx->f32_stage, bytes))) return rc;
    if ((rc = reserve(ctx, ctx->stage_a, sizeof(double) * 3 * (size_t)n))) return rc;
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->f32_stage.p, ctx->h_file, bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_widen_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float *)ctx->f32_stage.p, (int)n, 4,
                       (double *)ctx->stage_a.p);
    HIP_TRY(ctx, hipGetLastError());
    return icpmi_stream_push(ctx, (const double *)ctx->stage_a.p, n, voxel_size, min_points, cfg, result, error_history,
                             history_cap, info);
}

int icpmi_stream_push_host(icpmi_ctx *ctx, const double *raw_xyz, int64_t n_raw, double voxel_size, int64_t min_points,
                           const icpmi_config *cfg, icpmi_result *result, double *error_history, int32_t history_cap,
                           icpmi_stream_info *info)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!raw_xyz) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (n_raw <= 0 || n_raw > 700000000) return fail(ctx, ICPMI_ERR_ARG, "n_raw out of range");
    if ((rc = reserve(ctx, ctx->stage_a, sizeof(double) * 3 * (size_t)n_raw))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_a.p, raw_xyz, sizeof(double) * 3 * (size_t)n_raw, hipMemcpyHostToDevice, ctx->stream));
    return icpmi_stream_push(ctx, (const double *)ctx->stage_a.p, n_raw, voxel_size, min_points, cfg, result, error_history,
                             history_cap, info);
}

// ---- the map side of process_frame (slam_node.cpp:147-153, :211-221) -------------------------------------
void icpmi_grid_config_default(icpmi_grid_config *grid)
{
    if (!grid) return;
    grid->resolution = 0.2;   // slam_node.hpp:36-39
    grid->height_min = 0.3;
    grid->height_max = 2.0;
    grid->max_range = 40.0;
}

int icpmi_occupancy_update_device(icpmi_ctx *ctx, const double *d_world_xyz, int64_t n, const double sensor_xyz[3],
                                  const icpmi_grid_config *grid, int64_t *n_cells)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if ((!d_world_xyz && n != 0) || !sensor_xyz || !grid) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (n < 0 || n > 700000000) return fail(ctx, ICPMI_ERR_ARG, "n out of range");
    Range range("icpmi:occupancy_update");
    if ((rc = grid_update_queue(ctx, d_world_xyz, (int)n, sensor_xyz, grid))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    grid_finish(ctx);
    if (n_cells) *n_cells = ctx->grid_n;
    return ICPMI_OK;
}

int icpmi_occupancy_update(icpmi_ctx *ctx, const double *world_xyz, int64_t n, const double sensor_xyz[3],
                           const icpmi_grid_config *grid, int64_t *n_cells)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if ((!world_xyz && n != 0) || !sensor_xyz || !grid) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (n < 0 || n > 700000000) return fail(ctx, ICPMI_ERR_ARG, "n out of range");
    if ((rc = reserve(ctx, ctx->world, sizeof(double) * 3 * (size_t)std::max<int64_t>(n, 1)))) return rc;
    if (n > 0)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->world.p, world_xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    return icpmi_occupancy_update_device(ctx, (const double *)ctx->world.p, n, sensor_xyz, grid, n_cells);
}

int icpmi_occupancy_cells(icpmi_ctx *ctx, int32_t *cells_xy, int64_t cap_cells, int64_t *n_cells)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!n_cells) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    *n_cells = ctx->grid_n;
    if (!cells_xy || ctx->grid_n == 0) return ICPMI_OK;
    if (cap_cells < ctx->grid_n)
        return fail(ctx, ICPMI_ERR_CAPACITY, "output holds %lld cells, needs %lld", (long long)cap_cells, (long long)ctx->grid_n);
    const int n = (int)ctx->grid_n;
    if ((rc = reserve(ctx, ctx->grid_out, sizeof(int) * 2 * (size_t)n))) return rc;
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_grid_decode, dim3((n + 255) / 256), dim3(256), 0, s, (const unsigned long long *)ctx->grid_set.p, n,
                       (int *)ctx->grid_out.p);
    HIP_TRY(ctx, hipMemcpyAsync(cells_xy, ctx->grid_out.p, sizeof(int) * 2 * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

int icpmi_occupancy_clear(icpmi_ctx *ctx)
{
    if (!ctx) return ICPMI_ERR_NULL;
    ctx->grid_n = 0;
    return ICPMI_OK;
}

int icpmi_stream_current_scan(icpmi_ctx *ctx, double *out_xyz, int64_t cap, int64_t *n_out)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!n_out) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (ctx->stream_prev_n < 0) return fail(ctx, ICPMI_ERR_ARG, "no resident frame: call icpmi_stream_push first");
    *n_out = ctx->stream_prev_n;
    if (!out_xyz || ctx->stream_prev_n == 0) return ICPMI_OK;
    if (cap < ctx->stream_prev_n)
        return fail(ctx, ICPMI_ERR_CAPACITY, "output holds %lld rows, needs %lld", (long long)cap, (long long)ctx->stream_prev_n);
    HIP_TRY(ctx, hipMemcpyAsync(out_xyz, ctx->stream_prev.p, sizeof(double) * 3 * (size_t)ctx->stream_prev_n, hipMemcpyDeviceToHost,
                                ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ICPMI_OK;
}

int icpmi_stream_map_update(icpmi_ctx *ctx, const double pose[16], const icpmi_grid_config *grid, double *world_out,
                            int64_t world_cap, int64_t *n_world, int64_t *n_cells)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!pose) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (ctx->stream_prev_n < 0) return fail(ctx, ICPMI_ERR_ARG, "no resident frame: call icpmi_stream_push first");
    const int n = (int)ctx->stream_prev_n;
    if (n_world) *n_world = n;
    if (world_out && world_cap < n)
        return fail(ctx, ICPMI_ERR_CAPACITY, "world_out holds %lld rows, needs %d", (long long)world_cap, n);
    Range range("icpmi:map_update");
    hipStream_t s = ctx->stream;
    if ((rc = reserve(ctx, ctx->world, sizeof(double) * 3 * (size_t)std::max(n, 1)))) return rc;
    if (n > 0) {
        // world = curr * R^T + t^T (slam_node.cpp:147), the resident filtered scan -> ctx->world
        memset(ctx->h_state, 0, sizeof(IcpState));
        memcpy(ctx->h_state->total, pose, sizeof(double) * 16);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_state, ctx->h_state, sizeof(IcpState), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_transform, dim3(std::min(2048, (n + 255) / 256)), dim3(256), 0, s, (const double *)ctx->stream_prev.p,
                           (double *)ctx->world.p, n, ctx->d_state, 1, 0);
        if (world_out)
            HIP_TRY(ctx, hipMemcpyAsync(world_out, ctx->world.p, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, s));
    }
    if (grid) {
        const double sensor[3] = {pose[3], pose[7], pose[11]}; // new_pose.t() (slam_node.cpp:153)
        if ((rc = grid_update_queue(ctx, (const double *)ctx->world.p, n, sensor, grid))) return rc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));   // the call's one wait: world points and the set's size
    HIP_TRY(ctx, hipGetLastError());
    if (grid) grid_finish(ctx);
    if (n_cells) *n_cells = ctx->grid_n;
    return ICPMI_OK;
}

int icpmi_scan_context(icpmi_ctx *ctx, const double *cloud_xyz, int64_t n, double *desc_out)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!cloud_xyz || !desc_out) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (n < 0 || n > 700000000) return fail(ctx, ICPMI_ERR_ARG, "n out of range");
    const size_t bytes = sizeof(double) * 3 * (size_t)std::max<int64_t>(n, 1);
    if ((rc = reserve(ctx, ctx->stage_a, bytes))) return rc;
    if ((rc = reserve(ctx, ctx->vox_out, sizeof(double) * kScCells))) return rc;
    hipStream_t s = ctx->stream;
    if (n > 0) HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_a.p, cloud_xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_scan_context, dim3(1), dim3(1024), 0, s, (const double *)ctx->stage_a.p, (int)n,
                       (double *)ctx->vox_out.p);
    HIP_TRY(ctx, hipMemcpyAsync(desc_out, ctx->vox_out.p, sizeof(double) * kScCells, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

int icpmi_scan_context_distances(icpmi_ctx *ctx, const double *query_desc, const double *hist_descs,
                                 int64_t count, double *dist_out)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!query_desc || (count > 0 && (!hist_descs || !dist_out))) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (count < 0 || count > 100000000) return fail(ctx, ICPMI_ERR_ARG, "count out of range");
    if (count == 0) return ICPMI_OK;
    const size_t hb = sizeof(double) * kScCells * (size_t)count;
    if ((rc = reserve(ctx, ctx->stage_a, hb))) return rc;
    if ((rc = reserve(ctx, ctx->stage_b, sizeof(double) * kScCells))) return rc;
    if ((rc = reserve(ctx, ctx->vox_out, sizeof(double) * (size_t)count))) return rc;
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_a.p, hist_descs, hb, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_b.p, query_desc, sizeof(double) * kScCells, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_sc_distances, dim3((unsigned)count), dim3(64), 0, s, (const double *)ctx->stage_b.p,
                       (const double *)ctx->stage_a.p, (int)count, (double *)ctx->vox_out.p);
    HIP_TRY(ctx, hipMemcpyAsync(dist_out, ctx->vox_out.p, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

int icpmi_scan_context_distances_shift(icpmi_ctx *ctx, const double *query_desc, const double *hist_descs,
                                       int64_t count, double *dist_out, int32_t *shift_out)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!query_desc || (count > 0 && (!hist_descs || !dist_out || !shift_out))) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (count < 0 || count > 100000000) return fail(ctx, ICPMI_ERR_ARG, "count out of range");
    if (count == 0) return ICPMI_OK;
    const size_t hb = sizeof(double) * kScCells * (size_t)count;
    if ((rc = reserve(ctx, ctx->stage_a, hb))) return rc;
    if ((rc = reserve(ctx, ctx->stage_b, sizeof(double) * kScCells))) return rc;
    if ((rc = reserve(ctx, ctx->vox_out, (sizeof(double) + sizeof(int32_t)) * (size_t)count))) return rc;
    double *d_dist = (double *)ctx->vox_out.p;
    int32_t *d_shift = (int32_t *)(d_dist + count);
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_a.p, hist_descs, hb, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_b.p, query_desc, sizeof(double) * kScCells, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_sc_distances_shift, dim3((unsigned)count), dim3(64), 0, s, (const double *)ctx->stage_b.p,
                       (const double *)ctx->stage_a.p, (int)count, d_dist, d_shift);
    HIP_TRY(ctx, hipMemcpyAsync(dist_out, d_dist, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(shift_out, d_shift, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

int icpmi_sc_shift_transform(int32_t shift, double T[16])
{
    if (!T) return ICPMI_ERR_NULL;
    if (shift < 0 || shift >= kScSectors) return ICPMI_ERR_ARG;
    const double angle = shift * (2.0 * M_PI / 60);
    const double c = cos(angle), s = sin(angle);
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
    T[0] = c;
    T[1] = 0.0 - s; // (+0 at shift 0: the exact identity)
    T[4] = s;
    T[5] = c;
    return ICPMI_OK;
}

int icpmi_comm_unique_id(icpmi_ctx *ctx, void *id_out)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!id_out) return fail(ctx, ICPMI_ERR_NULL, "id_out is NULL");
    if ((rc = load_rccl(ctx))) return rc;
    static_assert(sizeof(ncclUniqueId) == ICPMI_UNIQUE_ID_BYTES, "unique id size");
    ncclUniqueId id;
    RCCL_TRY(ctx, ctx->rccl.GetUniqueId(&id));
    memcpy(id_out, &id, sizeof(id));
    return ICPMI_OK;
}

int icpmi_comm_init(icpmi_ctx *ctx, int32_t n_ranks, int32_t rank, const void *id)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(ctx, ICPMI_ERR_ARG, "bad rank %d of %d", rank, n_ranks);
    if (ctx->comm) return fail(ctx, ICPMI_ERR_ARG, "communicator already initialised");
    if (n_ranks == 1 && !id) { // no communicator wanted
        ctx->n_ranks = 1;
        ctx->rank = 0;
        return ICPMI_OK;
    }
    // (a 1-rank communicator is allowed: it runs the full sharded path, exchanges included)
    if (!id) return fail(ctx, ICPMI_ERR_NULL, "id is NULL");
    if ((rc = load_rccl(ctx))) return rc;
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    RCCL_TRY(ctx, ctx->rccl.CommInitRank(&ctx->comm, n_ranks, uid, rank));
    ctx->n_ranks = n_ranks;
    ctx->rank = rank;
    return ICPMI_OK;
}

int icpmi_comm_init_callbacks(icpmi_ctx *ctx, int32_t n_ranks, int32_t rank,
                              icpmi_allreduce_fn allreduce, icpmi_allgather_fn allgather, void *user)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(ctx, ICPMI_ERR_ARG, "bad rank %d of %d", rank, n_ranks);
    if (ctx->comm || ctx->cb_allreduce) return fail(ctx, ICPMI_ERR_ARG, "communicator already initialised");
    if (n_ranks > 1 && (!allreduce || !allgather)) return fail(ctx, ICPMI_ERR_NULL, "callback is NULL");
    ctx->cb_allreduce = allreduce;
    ctx->cb_allgather = allgather;
    ctx->cb_user = user;
    ctx->n_ranks = n_ranks;
    ctx->rank = rank;
    return ICPMI_OK;
}

// Who is in the communicator, asked of the communicator itself: its size and this rank from RCCL (ncclCommCount,
// ncclCommUserRank, ncclCommCuDevice), and every rank's device ordinal and PCI bus id gathered through the library's own
// all-gather -- the exchange the sharded normals use.  A collective: every rank must call it.
int icpmi_comm_info(icpmi_ctx *ctx, icpmi_comm_info_t *out)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!out) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    memset(out, 0, sizeof(*out));
    out->kind = ctx->comm ? 1 : (ctx->cb_allreduce ? 2 : 0);
    out->n_ranks = ctx->n_ranks;
    out->rank = ctx->rank;
    int device = ctx->opt.device;
    if (ctx->comm) {
        int v = 0;
        RCCL_TRY(ctx, ctx->rccl.CommCount(ctx->comm, &v));
        out->n_ranks = v;
        RCCL_TRY(ctx, ctx->rccl.CommUserRank(ctx->comm, &v));
        out->rank = v;
        RCCL_TRY(ctx, ctx->rccl.CommCuDevice(ctx->comm, &device));
    }
    const int nr = out->n_ranks;
    if (nr > ICPMI_MAX_RANKS_INFO) return fail(ctx, ICPMI_ERR_ARG, "more than %d ranks", ICPMI_MAX_RANKS_INFO);
    // one record of four doubles per rank: {device ordinal, 16 characters of PCI bus id, 0}
    constexpr size_t per = 4;
    double rec[per] = {0.0, 0.0, 0.0, 0.0};
    char bus[32] = {0};
    HIP_TRY(ctx, hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device));
    rec[0] = (double)device;
    memcpy(&rec[1], bus, 16);
    if ((rc = reserve(ctx, ctx->stage_c, sizeof(double) * per * (size_t)nr))) return rc;
    double *d = (double *)ctx->stage_c.p;
    HIP_TRY(ctx, hipMemsetAsync(d, 0, sizeof(double) * per * (size_t)nr, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d + per * (size_t)out->rank, rec, sizeof(rec), hipMemcpyHostToDevice, ctx->stream));
    if (out->kind != 0 && (rc = exchange_allgather(ctx, d, per))) return rc;
    std::vector<double> host(per * (size_t)nr);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), d, sizeof(double) * host.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int r = 0; r < nr; ++r) {
        out->device[r] = (int32_t)host[per * r];
        memcpy(out->pci_bus_id[r], &host[per * r + 1], 16);
        out->pci_bus_id[r][15] = '\0';
    }
    return ICPMI_OK;
}

int icpmi_comm_finalize(icpmi_ctx *ctx)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (ctx->comm) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        RCCL_TRY(ctx, ctx->rccl.CommDestroy(ctx->comm));
        ctx->comm = nullptr;
    }
    ctx->cb_allreduce = nullptr;
    ctx->cb_allgather = nullptr;
    ctx->cb_user = nullptr;
    ctx->n_ranks = 1;
    ctx->rank = 0;
    return ICPMI_OK;
}

int icpmi_reset_profile(icpmi_ctx *ctx)
{
    if (!ctx) return ICPMI_ERR_NULL;
    if (ctx->ev_used) { // events of finished calls not read yet: they belong to what is being discarded
        (void)hipSetDevice(ctx->opt.device);
        (void)hipStreamSynchronize(ctx->stream);
        harvest_profile(ctx);
    }
    memset(&ctx->prof, 0, sizeof(ctx->prof));
    return ICPMI_OK;
}

int icpmi_get_profile(icpmi_ctx *ctx, icpmi_profile *out)
{
    if (!ctx || !out) return ICPMI_ERR_NULL;
    if (ctx->ev_used) { // the events of the calls since the last look are read now (see align_device)
        (void)hipSetDevice(ctx->opt.device);
        (void)hipStreamSynchronize(ctx->stream);
        harvest_profile(ctx);
    }
    *out = ctx->prof;
    out->coarse_minima_bytes = (int64_t)ctx->coarse.cap;
    return ICPMI_OK;
}

// the rows of the last registration as the loop left them -- matches, moved coordinates, and the order the rows were taken
// in (0..n-1 when they were not sorted): scripts/loop_rows.py, tests/test_gpu_nn_reuse.py, tests/test_gpu_loop_matches.py.
// `n` must be the last registration's row count (ICPMI_ERR_ARG otherwise, and when none has completed).  Returns
// ICPMI_DEBUG_NO_IDX (1) when idx does not hold the last pass's matches -- the small-cloud kernel's loop, or a nearest_batch
// call since -- with idx_out set to -1: cur_out and perm_out are still the last pass's.
constexpr int ICPMI_DEBUG_NO_IDX = 1;
extern "C" int icpmi_debug_loop_rows(icpmi_ctx *ctx, int32_t *idx_out, double *cur_out, uint32_t *perm_out, int64_t n)
{
    if (!ctx || n < 0 || n != ctx->loop_rows || (size_t)n * sizeof(int) > ctx->idx.cap || (size_t)n * 24 > ctx->cur.cap)
        return ICPMI_ERR_ARG;
    if (hipDeviceSynchronize() != hipSuccess) return ICPMI_ERR_HIP;
    if (!ctx->loop_idx_valid)
        for (int64_t i = 0; i < n; ++i) idx_out[i] = -1;
    else if (hipMemcpy(idx_out, ctx->idx.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return ICPMI_ERR_HIP;
    if (hipMemcpy(cur_out, ctx->cur.p, (size_t)n * 24, hipMemcpyDeviceToHost) != hipSuccess) return ICPMI_ERR_HIP;
    const SortPlanes sp(ctx->src_sort.p, (size_t)n);
    if (ctx->loop_sorted && ctx->src_sort.p && ctx->src_sort.cap >= sp.bytes) {
        if (hipMemcpy(perm_out, sp.perm, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return ICPMI_ERR_HIP;
    } else {
        for (int64_t i = 0; i < n; ++i) perm_out[i] = (uint32_t)i;
    }
    return ctx->loop_idx_valid ? ICPMI_OK : ICPMI_DEBUG_NO_IDX;
}

// List reuse of the last registration with profiling on (RowBounds, kernels.h): per bounded pass, the rows listed by its
// coarse pass and the workgroup columns that pass ran.  Returns the number of passes (at most `cap` are written), 0 without
// list reuse or profiling.
extern "C" int64_t icpmi_debug_nn_reuse(const icpmi_ctx *ctx, uint32_t *rows_out, uint32_t *blocks_out, int64_t cap)
{
    if (!ctx) return 0;
    const int64_t np = (int64_t)ctx->reuse_rows.size();
    for (int64_t p = 0; p < np && p < cap; ++p) {
        if (rows_out) rows_out[p] = ctx->reuse_rows[p];
        if (blocks_out) blocks_out[p] = ctx->reuse_blocks[p];
    }
    return np;
}

// The match margin of the last registration with profiling on (list_reuse.h): per bounded pass, the rows whose kept match
// was certified and that were neither listed nor scanned.  Returns the number of passes (at most `cap` are written), 0
// where the margin was off (ICPMI_NN_MARGIN=0, no list reuse, another resolve kernel) or without profiling.
extern "C" int64_t icpmi_debug_nn_margin(const icpmi_ctx *ctx, uint32_t *rows_out, int64_t cap)
{
    if (!ctx) return 0;
    const int64_t np = (int64_t)ctx->margin_rows.size();
    for (int64_t p = 0; p < np && p < cap; ++p)
        if (rows_out) rows_out[p] = ctx->margin_rows[p];
    return np;
}

} // extern "C"

// ======================================================================================================================
// Pose graph (core/pose_graph.cpp): factors and estimates on the host, the LM iteration on the device (pose_graph.h).
// The LM policy below restates LevenbergMarquardtOptimizer::tryLambda / iterate and NonlinearOptimizer::defaultOptimize
// exactly as scripts/pose_graph_ref.py levenberg_marquardt does, rule for rule.

// The graph's structure for the device solve (rebuilt by every optimize(): O(poses + factors) on the host).
struct PgPlan {
    int n = 0, F = 0, nb = 0, nseg = 0, nblocks = 0, nloops = 0;
    int max_seg = 0;                     // nodes of the longest segment
    bool loss = false;                   // the loss is on and the graph has a loop factor: the kernels of pose_graph_loss.h
    bool info = false;                   // the graph has an information factor: the kernels of pose_graph_info.h
    std::vector<int32_t> keys, map;
};

struct icpmi_pose_graph {
    icpmi_ctx *ctx = nullptr;
    icpmi_pose_graph_config cfg;
    std::vector<PgFactor> factors;
    std::vector<double> init;            // 12 per pose index (valid where has_init)
    std::vector<char> has_init;
    std::vector<double> opt;             // optimised values, 12 per pose index (valid where has_init, while optimized)
    int64_t num_poses = 0, num_loops = 0;
    bool optimized = false;
    int32_t loss_kind = ICPMI_PG_LOSS_NONE;   // on the loop-closure factors (pose_graph_loss.h)
    double loss_scale = 0.0;
    bool values_on_device = false;       // d_X, d_fac, d_map and d_rank are those of the last optimize()
    int opt_factors = 0;                 // factors and loop factors of that optimize()
    int64_t opt_loops = 0;
    size_t uploaded_factors = 0;         // factors already in d_fac
    // full-information factors (pose_graph_info.h): info_slot[f] = position of factor f's R among info_R's blocks of 21
    // doubles, -1 for a diagonal factor.  Both go up incrementally, and only once the graph holds an information factor.
    std::vector<int32_t> info_slot;
    std::vector<double> info_R;
    size_t uploaded_slots = 0, uploaded_R = 0;   // entries of info_slot in d_slot, doubles of info_R in d_infoR
    int64_t init_dirty_lo = INT64_MAX, init_dirty_hi = 0;   // pose range of estimates not yet in d_init
    DevBuf d_fac, d_init, d_map, d_keys, d_X, d_Xc, d_A, d_rw, d_err, d_H, d_g, d_D, d_gn, d_Cn, d_L, d_U, d_Y,
        d_schur, d_S, d_xb, d_delta, d_errc, d_errl, d_out, d_status, d_inc_ptr, d_inc, d_cn_ptr, d_cn, d_segs,
        d_blocks, d_codes, d_sep_node, d_sep_segs, d_sep_pos, d_node_seg, d_rank, d_wd, d_slot, d_infoR;
    double *h_out = nullptr;             // pinned: the two sums and the status of a trial
    // marginal covariances (pose_graph_marginals.h): the plan of the last optimize(), and whether d_L / d_U / d_Y / d_S
    // hold the lam = 0 factorisation at d_X (cleared by every add, optimize() and set_loop_loss)
    PgPlan plan;
    bool marg_factored = false;
    DevBuf d_mq, d_mW, d_mblk, d_mX, d_mout;
    icpmi_pose_graph_info last{};        // of the last optimize()
};

namespace {

int pg_check_T(icpmi_ctx *ctx, const double *T)
{
    if (!T) return fail(ctx, ICPMI_ERR_NULL, "null transform");
    for (int e = 0; e < 16; ++e)
        if (!std::isfinite(T[e])) return fail(ctx, ICPMI_ERR_ARG, "non-finite transform entry");
    return ICPMI_OK;
}

void pg_to12(const double *T, double *o) // row-major 4x4 -> R (9), t (3); rotations taken as given (Rot3(Matrix3))
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) o[3 * r + c] = T[4 * r + c];
    o[9] = T[3]; o[10] = T[7]; o[11] = T[11];
}
void pg_to16(const double *o, double *T)
{
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[4 * r + c] = o[3 * r + c];
        T[4 * r + 3] = o[9 + r];
    }
    T[12] = T[13] = T[14] = 0.0;
    T[15] = 1.0;
}

void pg_grow(icpmi_pose_graph *g, int64_t idx)
{
    if ((int64_t)g->has_init.size() <= idx) {
        g->has_init.resize(idx + 1, 0);
        g->init.resize(12 * (size_t)(idx + 1), 0.0);
    }
}
void pg_set_init(icpmi_pose_graph *g, int64_t idx, const double *p12)
{
    pg_grow(g, idx);
    std::copy(p12, p12 + 12, g->init.begin() + 12 * idx);
    g->has_init[idx] = 1;
    g->init_dirty_lo = std::min(g->init_dirty_lo, idx);
    g->init_dirty_hi = std::max(g->init_dirty_hi, idx + 1);
    g->num_poses = std::max(g->num_poses, idx + 1);
}
bool pg_has(const icpmi_pose_graph *g, int64_t idx)
{
    return idx >= 0 && idx < (int64_t)g->has_init.size() && g->has_init[idx];
}

void pg_factor(PgFactor &f, int kind, int64_t i, int64_t j, const double *T, double rs, double ts)
{
    f.kind = kind;
    f.i = (int32_t)i;
    f.j = (int32_t)j;
    f.reserved = 0;                       // 1: a loop closure (pose_graph_loss.h)
    pg_to12(T, f.Z);
    for (int a = 0; a < 3; ++a) {
        f.inv_sigma[a] = 1.0 / rs;        // noiseModel::Diagonal::Sigmas keeps 1/sigma and whitens by multiplying
        f.inv_sigma[3 + a] = 1.0 / ts;
    }
}

// the information matrix of a new factor -> R's upper triangle, or ICPMI_ERR_ARG with the reason
int pg_factor_information(icpmi_ctx *ctx, const double *info, double *R21)
{
    switch (pg_info_cholesky(info, R21)) {
    case kPgInfoOk: return ICPMI_OK;
    case kPgInfoNotFinite: return fail(ctx, ICPMI_ERR_ARG, "non-finite information matrix entry");
    case kPgInfoAsymmetric: return fail(ctx, ICPMI_ERR_ARG, "the information matrix is not symmetric");
    default: return fail(ctx, ICPMI_ERR_ARG, "the information matrix is not positive definite (a Cholesky pivot is not > 0)");
    }
}

// the slot of the factor just pushed: R21 null for a diagonal factor
void pg_push_slot(icpmi_pose_graph *g, const double *R21)
{
    if (!R21) {
        g->info_slot.push_back(-1);
        return;
    }
    g->info_slot.push_back((int32_t)(g->info_R.size() / 21));
    g->info_R.insert(g->info_R.end(), R21, R21 + 21);
}

template <class T> int pg_upload(icpmi_ctx *ctx, DevBuf &b, const std::vector<T> &v)
{
    int rc;
    if ((rc = reserve(ctx, b, sizeof(T) * std::max<size_t>(v.size(), 1)))) return rc;
    if (!v.empty()) HIP_TRY(ctx, hipMemcpyAsync(b.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, ctx->stream));
    return ICPMI_OK;
}

unsigned pg_grid(size_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }

int pg_plan(icpmi_pose_graph *g, PgPlan &P)
{
    icpmi_ctx *ctx = g->ctx;
    const int64_t np = g->num_poses;
    P.map.assign(np, -1);
    for (int64_t k = 0; k < np; ++k)
        if (g->has_init[k]) {
            P.map[k] = (int32_t)P.keys.size();
            P.keys.push_back((int32_t)k);
        }
    const int n = (int)P.keys.size(), F = (int)g->factors.size();
    P.n = n;
    P.F = F;
    std::vector<char> sep(n, 0);
    std::vector<int32_t> inc_cnt(n + 1, 0), cn_cnt(n + 1, 0);
    for (int k = 0; k < n; ++k)
        if (P.keys[k] % kPgChainK == kPgChainK - 1) sep[k] = 1;        // caps a chain run at K - 1 nodes
    for (int f = 0; f < F; ++f) {
        const PgFactor &fa = g->factors[f];
        inc_cnt[P.map[fa.i] + 1]++;
        if (fa.kind == 1) {
            inc_cnt[P.map[fa.j] + 1]++;
            if (fa.j == fa.i + 1) cn_cnt[P.map[fa.i] + 1]++;          // chain factor (k, k+1)
            else sep[P.map[fa.i]] = sep[P.map[fa.j]] = 1;             // any other between factor: two separators
        }
    }
    for (int k = 0; k < n; ++k) {
        inc_cnt[k + 1] += inc_cnt[k];
        cn_cnt[k + 1] += cn_cnt[k];
    }
    std::vector<int32_t> inc(inc_cnt[n]), cn(cn_cnt[n]), ip(inc_cnt.begin(), inc_cnt.end() - 1),
        cp(cn_cnt.begin(), cn_cnt.end() - 1);
    for (int f = 0; f < F; ++f) {   // ascending f within every node
        const PgFactor &fa = g->factors[f];
        inc[ip[P.map[fa.i]]++] = 2 * f;
        if (fa.kind == 1) {
            inc[ip[P.map[fa.j]]++] = 2 * f + 1;
            if (fa.j == fa.i + 1) cn[cp[P.map[fa.i]]++] = f;
        }
    }
    // separators in compact order; segments = maximal runs of the rest
    std::vector<int32_t> sep_pos(n, -1), sep_node, node_seg(n), sep_segs;
    std::vector<PgSeg> segs;
    for (int k = 0; k < n; ++k)
        if (sep[k]) {
            sep_pos[k] = (int32_t)sep_node.size();
            sep_node.push_back(k);
        }
    const int nb = (int)sep_node.size();
    sep_segs.assign(2 * (size_t)nb, -1);
    for (int k = 0; k < n;) {
        if (sep[k]) {
            node_seg[k] = -1 - sep_pos[k];
            ++k;
            continue;
        }
        PgSeg s;
        s.start = k;
        while (k < n && !sep[k]) node_seg[k++] = (int32_t)segs.size();
        s.len = k - s.start;
        s.left = s.start > 0 ? s.start - 1 : -1;
        s.right = k < n ? k : -1;
        if (s.left >= 0) sep_segs[2 * sep_pos[s.left] + 1] = (int32_t)segs.size();
        if (s.right >= 0) sep_segs[2 * sep_pos[s.right]] = (int32_t)segs.size();
        segs.push_back(s);
    }
    // the reduced system's lower blocks and what each sums, in a fixed order
    std::vector<std::vector<int32_t>> per;                 // contributions per block
    std::vector<PgBlock> blocks;
    std::vector<std::pair<int64_t, int32_t>> index;        // (row * nb + col) -> block, sorted later
    auto block = [&](int row, int col) -> std::vector<int32_t> & {
        const int64_t key = (int64_t)row * nb + col;
        for (auto it = index.rbegin(); it != index.rend() && it - index.rbegin() < 4; ++it)
            if (it->first == key) return per[it->second];
        index.push_back({key, (int32_t)blocks.size()});
        PgBlock b{row, col, 0, 0};
        blocks.push_back(b);
        per.emplace_back();
        return per.back();
    };
    for (int a = 0; a < nb; ++a) {
        auto &c = block(a, a);
        const int v = sep_node[a];
        c.push_back(v);                                            // D_v + lam I
        if (sep_segs[2 * a] >= 0) c.push_back((4 << 28) | (4 * sep_segs[2 * a] + 3));          // RR of the left segment
        if (sep_segs[2 * a + 1] >= 0) c.push_back((4 << 28) | (4 * sep_segs[2 * a + 1] + 0));  // LL of the right one
        if (v + 1 < n && sep[v + 1] && cn_cnt[v + 1] > cn_cnt[v]) block(a + 1, a).push_back((1 << 28) | v);
    }
    for (size_t s = 0; s < segs.size(); ++s)
        if (segs[s].left >= 0 && segs[s].right >= 0)
            block(sep_pos[segs[s].right], sep_pos[segs[s].left]).push_back((4 << 28) | (4 * (int)s + 1));
    // non-chain between factors: O(1) amortised lookup of the (row, col) block through a sorted index
    {
        std::vector<std::pair<int64_t, int32_t>> sorted(index);
        std::sort(sorted.begin(), sorted.end());
        std::vector<std::pair<int64_t, int32_t>> extra;
        for (int f = 0; f < F; ++f) {
            const PgFactor &fa = g->factors[f];
            if (fa.kind != 1 || fa.j == fa.i + 1) continue;
            const int pi = sep_pos[P.map[fa.i]], pj = sep_pos[P.map[fa.j]];
            const int row = std::max(pi, pj), col = std::min(pi, pj);
            const int64_t key = (int64_t)row * nb + col;
            auto it = std::lower_bound(sorted.begin(), sorted.end(), std::make_pair(key, (int32_t)-1));
            int32_t bidx;
            if (it != sorted.end() && it->first == key) bidx = it->second;
            else {
                bidx = (int32_t)blocks.size();
                blocks.push_back(PgBlock{row, col, 0, 0});
                per.emplace_back();
                sorted.insert(it, {key, bidx});
            }
            per[bidx].push_back(((pi > pj ? 3 : 2) << 28) | f);
        }
    }
    std::vector<int32_t> rank(F, -1);                      // loop factors in add_loop_closure order
    for (int f = 0; f < F; ++f)
        if (g->factors[f].reserved == 1) rank[f] = P.nloops++;
    P.loss = g->loss_kind != ICPMI_PG_LOSS_NONE && P.nloops > 0;
    P.info = !g->info_R.empty();
    std::vector<int32_t> codes;
    for (size_t b = 0; b < blocks.size(); ++b) {
        blocks[b].begin = (int32_t)codes.size();
        codes.insert(codes.end(), per[b].begin(), per[b].end());
        blocks[b].end = (int32_t)codes.size();
    }
    if (F >= (1 << 28) || n >= (1 << 26)) return fail(ctx, ICPMI_ERR_ARG, "pose graph too large for the block codes");
    P.nb = nb;
    P.nseg = (int)segs.size();
    for (const PgSeg &sg : segs) P.max_seg = std::max(P.max_seg, (int)sg.len);
    P.nblocks = (int)blocks.size();
    int rc;
    if ((rc = pg_upload(ctx, g->d_map, P.map)) || (rc = pg_upload(ctx, g->d_keys, P.keys)) ||
        (rc = pg_upload(ctx, g->d_inc_ptr, inc_cnt)) || (rc = pg_upload(ctx, g->d_inc, inc)) ||
        (rc = pg_upload(ctx, g->d_cn_ptr, cn_cnt)) || (rc = pg_upload(ctx, g->d_cn, cn)) ||
        (rc = pg_upload(ctx, g->d_segs, segs)) || (rc = pg_upload(ctx, g->d_blocks, blocks)) ||
        (rc = pg_upload(ctx, g->d_codes, codes)) || (rc = pg_upload(ctx, g->d_sep_node, sep_node)) ||
        (rc = pg_upload(ctx, g->d_sep_segs, sep_segs)) || (rc = pg_upload(ctx, g->d_sep_pos, sep_pos)) ||
        (rc = pg_upload(ctx, g->d_node_seg, node_seg)) || (rc = pg_upload(ctx, g->d_rank, rank)))
        return rc;
    const size_t F1 = std::max(F, 1), n1 = std::max(n, 1), nr = 6 * (size_t)std::max(nb, 1);
    struct { DevBuf *b; size_t bytes; } need[] = {
        {&g->d_X, 96 * n1}, {&g->d_Xc, 96 * n1}, {&g->d_A, 576 * F1}, {&g->d_rw, 48 * F1}, {&g->d_err, 8 * F1},
        {&g->d_H, 864 * F1}, {&g->d_g, 96 * F1}, {&g->d_D, 288 * n1}, {&g->d_gn, 48 * n1}, {&g->d_Cn, 288 * n1},
        {&g->d_L, 288 * n1}, {&g->d_U, 288 * n1}, {&g->d_Y, 624 * n1}, {&g->d_schur, 1248 * (size_t)std::max(P.nseg, 1)},
        {&g->d_S, 8 * nr * nr}, {&g->d_xb, 8 * nr}, {&g->d_delta, 48 * n1}, {&g->d_errc, 8 * F1}, {&g->d_errl, 8 * F1},
        {&g->d_out, 64}, {&g->d_status, 64}, {&g->d_wd, 16 * (size_t)std::max(P.nloops, 1)}};
    for (auto &q : need)
        if ((rc = reserve(ctx, *q.b, q.bytes))) return rc;
    return ICPMI_OK;
}

// one readback: {sum a, sum b, status}
int pg_sums(icpmi_pose_graph *g, const double *a, const double *b, int F, double out[3])
{
    icpmi_ctx *ctx = g->ctx;
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_pg_reduce, dim3(1), dim3(1024), 0, s, a, b, F, (double *)g->d_out.p);
    HIP_TRY(ctx, hipMemcpyAsync(g->h_out, g->d_out.p, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(g->h_out + 2, g->d_status.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipGetLastError());
    out[0] = g->h_out[0];
    out[1] = g->h_out[1];
    int st;
    memcpy(&st, g->h_out + 2, sizeof(int));
    out[2] = st;
    return ICPMI_OK;
}

// (H + lam I) delta = -g on the device; then the candidate and its two errors
int pg_trial(icpmi_pose_graph *g, const PgPlan &P, const PgLin &lin, double lam, double out[3])
{
    icpmi_ctx *ctx = g->ctx;
    hipStream_t s = ctx->stream;
    const int n = P.n, F = P.F, nb = P.nb, nr = 6 * nb;
    HIP_TRY(ctx, hipMemsetAsync(g->d_status.p, 0, sizeof(int), s));
    int *status = (int *)g->d_status.p;
    if (P.nseg > 0)
        hipLaunchKernelGGL(k_pg_segment, dim3(P.nseg), dim3(kPgSegThreads), 0, s, (const PgSeg *)g->d_segs.p, lam,
                           (const double *)g->d_D.p, (const double *)g->d_gn.p, (const double *)g->d_Cn.p,
                           (double *)g->d_L.p, (double *)g->d_U.p, (double *)g->d_Y.p, (double *)g->d_schur.p, status);
    if (nb > 0) {
        double *S = (double *)g->d_S.p;
        HIP_TRY(ctx, hipMemsetAsync(S, 0, sizeof(double) * (size_t)nr * nr, s));   // blocks with no coupling are zero
        hipLaunchKernelGGL(k_pg_reduced, dim3(P.nblocks), dim3(64), 0, s, (const PgBlock *)g->d_blocks.p,
                           (const int32_t *)g->d_codes.p, nr, lam, (const double *)g->d_D.p, (const double *)g->d_Cn.p,
                           (const double *)lin.H, (const double *)g->d_schur.p, S);
        hipLaunchKernelGGL(k_pg_reduced_rhs, dim3(pg_grid(nr, 256)), dim3(256), 0, s, (const int32_t *)g->d_sep_node.p,
                           (const int32_t *)g->d_sep_segs.p, nb, (const double *)g->d_gn.p, (const double *)g->d_schur.p,
                           (double *)g->d_xb.p);
        for (int k0 = 0; k0 < nr; k0 += kCholNb) {
            hipLaunchKernelGGL(k_chol_diag, dim3(1), dim3(256), 0, s, S, nr, k0, status);
            const int rest = nr - k0 - kCholNb;
            if (rest <= 0) break;
            hipLaunchKernelGGL(k_chol_panel, dim3(pg_grid(rest, 64)), dim3(64), 0, s, S, nr, k0);
            const unsigned T = pg_grid(rest, 32);
            hipLaunchKernelGGL(k_chol_update, dim3(T, T), dim3(256), 0, s, S, nr, k0);
        }
        hipLaunchKernelGGL(k_trsv_pair, dim3(1), dim3(256), 0, s, (const double *)S, nr, (double *)g->d_xb.p);
    }
    hipLaunchKernelGGL(k_pg_backsub, dim3(pg_grid(6 * (size_t)n, 256)), dim3(256), 0, s, (const int32_t *)g->d_node_seg.p,
                       (const PgSeg *)g->d_segs.p, (const int32_t *)g->d_sep_pos.p, (const double *)g->d_Y.p,
                       (const double *)g->d_xb.p, n, (double *)g->d_delta.p);
    hipLaunchKernelGGL(k_pg_retract, dim3(pg_grid(n, 128)), dim3(128), 0, s, (const double *)g->d_X.p,
                       (const double *)g->d_delta.p, n, (double *)g->d_Xc.p);
    if (P.info)
        hipLaunchKernelGGL(k_pg_trial_info, dim3(pg_grid(F, 128)), dim3(128), 0, s, (const PgFactor *)g->d_fac.p,
                           (const int32_t *)g->d_slot.p, (const double *)g->d_infoR.p, (const int32_t *)g->d_map.p, F,
                           (const double *)g->d_Xc.p, lin, (const double *)g->d_delta.p,
                           P.loss ? (int)g->loss_kind : kPgLossNone, g->loss_scale, (double *)g->d_errc.p,
                           (double *)g->d_errl.p);
    else if (P.loss)
        hipLaunchKernelGGL(k_pg_trial_loss, dim3(pg_grid(F, 128)), dim3(128), 0, s, (const PgFactor *)g->d_fac.p,
                           (const int32_t *)g->d_map.p, F, (const double *)g->d_Xc.p, lin, (const double *)g->d_delta.p,
                           (int)g->loss_kind, g->loss_scale, (double *)g->d_errc.p, (double *)g->d_errl.p);
    else
        hipLaunchKernelGGL(k_pg_trial, dim3(pg_grid(F, 128)), dim3(128), 0, s, (const PgFactor *)g->d_fac.p,
                           (const int32_t *)g->d_map.p, F, (const double *)g->d_Xc.p, lin, (const double *)g->d_delta.p,
                           (double *)g->d_errc.p, (double *)g->d_errl.p);
    return pg_sums(g, (const double *)g->d_errc.p, (const double *)g->d_errl.p, F, out);
}

// error: the sum of lin.err, read back when asked for.  lin0: the linearised error at a zero step; without a loss it is
// the error itself and costs nothing, under a loss it is a sum of its own (per factor in d_errl, which the next trial
// overwrites) and always read back.
int pg_linearize(icpmi_pose_graph *g, const PgPlan &P, const PgLin &lin, double *error, double *lin0)
{
    icpmi_ctx *ctx = g->ctx;
    hipStream_t s = ctx->stream;
    if (P.info)
        hipLaunchKernelGGL(k_pg_linearize_info, dim3(pg_grid(P.F, kPgInfoThreads)), dim3(kPgInfoThreads), 0, s, (const PgFactor *)g->d_fac.p,
                           (const int32_t *)g->d_slot.p, (const double *)g->d_infoR.p, (const int32_t *)g->d_map.p, P.F,
                           (const double *)g->d_X.p, lin, P.loss ? (int)g->loss_kind : kPgLossNone, g->loss_scale,
                           P.loss ? (double *)g->d_errl.p : nullptr);
    else if (P.loss)
        hipLaunchKernelGGL(k_pg_linearize_loss, dim3(pg_grid(P.F, 128)), dim3(128), 0, s, (const PgFactor *)g->d_fac.p,
                           (const int32_t *)g->d_map.p, P.F, (const double *)g->d_X.p, lin, (int)g->loss_kind,
                           g->loss_scale, (double *)g->d_errl.p);
    else
        hipLaunchKernelGGL(k_pg_linearize, dim3(pg_grid(P.F, 128)), dim3(128), 0, s, (const PgFactor *)g->d_fac.p,
                           (const int32_t *)g->d_map.p, P.F, (const double *)g->d_X.p, lin);
    hipLaunchKernelGGL(k_pg_assemble, dim3(pg_grid(78 * (size_t)P.n, 256)), dim3(256), 0, s, lin,
                       (const int32_t *)g->d_inc_ptr.p, (const int32_t *)g->d_inc.p, (const int32_t *)g->d_cn_ptr.p,
                       (const int32_t *)g->d_cn.p, P.n, (double *)g->d_D.p, (double *)g->d_gn.p, (double *)g->d_Cn.p);
    if (P.loss) {
        double out[3];
        int rc = pg_sums(g, lin.err, (const double *)g->d_errl.p, P.F, out);
        if (error) *error = out[0];
        *lin0 = out[1];
        return rc;
    }
    if (!error) return ICPMI_OK;
    double out[3];
    int rc = pg_sums(g, lin.err, nullptr, P.F, out);
    *error = out[0];
    return rc;
}

// The lam = 0 factorisation of H at d_X for the marginal covariances (pose_graph_marginals.h): linearise, then the
// segment, reduced and Cholesky launches exactly as pg_trial makes them.  A non-positive pivot is the caller's graph.
int pg_marg_factorize(icpmi_pose_graph *g)
{
    icpmi_ctx *ctx = g->ctx;
    hipStream_t s = ctx->stream;
    const PgPlan &P = g->plan;
    PgLin lin{(double *)g->d_A.p, (double *)g->d_rw.p, (double *)g->d_err.p, (double *)g->d_H.p, (double *)g->d_g.p};
    const int nr = 6 * P.nb;
    const double lam = 0.0;
    double lin0 = 0.0;
    int rc;
    if ((rc = pg_linearize(g, P, lin, nullptr, &lin0))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(g->d_status.p, 0, sizeof(int), s));
    int *status = (int *)g->d_status.p;
    if (P.nseg > 0)
        hipLaunchKernelGGL(k_pg_segment, dim3(P.nseg), dim3(kPgSegThreads), 0, s, (const PgSeg *)g->d_segs.p, lam,
                           (const double *)g->d_D.p, (const double *)g->d_gn.p, (const double *)g->d_Cn.p,
                           (double *)g->d_L.p, (double *)g->d_U.p, (double *)g->d_Y.p, (double *)g->d_schur.p, status);
    if (P.nb > 0) {
        double *S = (double *)g->d_S.p;
        HIP_TRY(ctx, hipMemsetAsync(S, 0, sizeof(double) * (size_t)nr * nr, s));
        hipLaunchKernelGGL(k_pg_reduced, dim3(P.nblocks), dim3(64), 0, s, (const PgBlock *)g->d_blocks.p,
                           (const int32_t *)g->d_codes.p, nr, lam, (const double *)g->d_D.p, (const double *)g->d_Cn.p,
                           (const double *)lin.H, (const double *)g->d_schur.p, S);
        for (int k0 = 0; k0 < nr; k0 += kCholNb) {
            hipLaunchKernelGGL(k_chol_diag, dim3(1), dim3(256), 0, s, S, nr, k0, status);
            const int rest = nr - k0 - kCholNb;
            if (rest <= 0) break;
            hipLaunchKernelGGL(k_chol_panel, dim3(pg_grid(rest, 64)), dim3(64), 0, s, S, nr, k0);
            const unsigned T = pg_grid(rest, 32);
            hipLaunchKernelGGL(k_chol_update, dim3(T, T), dim3(256), 0, s, S, nr, k0);
        }
    }
    HIP_TRY(ctx, hipMemcpyAsync(g->h_out + 2, g->d_status.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipGetLastError());
    int st;
    memcpy(&st, g->h_out + 2, sizeof(int));
    if (st != 0)
        return fail(ctx, ICPMI_ERR_ARG, "the Gauss-Newton matrix met a non-positive pivot: the graph has no covariance "
                                        "(is a prior missing?)");
    g->marg_factored = true;
    return ICPMI_OK;
}

// the state rule of the covariance calls, as icpmi_pose_graph_loop_weights states it
int pg_marg_state(icpmi_pose_graph *g)
{
    if (!g->optimized || !g->values_on_device || (int64_t)g->factors.size() != g->opt_factors ||
        (int64_t)g->plan.map.size() != g->num_poses)
        return fail(g->ctx, ICPMI_ERR_ARG, "covariances need the optimised state of the last optimize()");
    return ICPMI_OK;
}

// the joint marginal covariance of q distinct poses into cov (6q x 6q, row-major)
int pg_marginals(icpmi_pose_graph *g, const int64_t *indices, int32_t q, double *cov)
{
    icpmi_ctx *ctx = g->ctx;
    int rc;
    if ((rc = pg_marg_state(g))) return rc;
    if (q <= 0) return fail(ctx, ICPMI_ERR_ARG, "a covariance query names at least one pose");
    if (q >= 46341) return fail(ctx, ICPMI_ERR_ARG, "a covariance query of %d poses is too large", (int)q);   // q^2 blocks
    const PgPlan &P = g->plan;
    std::vector<int32_t> qnode(q);
    for (int32_t a = 0; a < q; ++a) {
        if (!pg_has(g, indices[a]) || P.map[indices[a]] < 0)
            return fail(ctx, ICPMI_ERR_ARG, "Pose index %lld not found", (long long)indices[a]);
        qnode[a] = P.map[indices[a]];
    }
    {
        std::vector<int32_t> sorted(qnode);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(ctx, ICPMI_ERR_ARG, "a covariance query names a pose twice");
    }
    if (!g->marg_factored && (rc = pg_marg_factorize(g))) return rc;
    hipStream_t s = ctx->stream;
    const size_t nr = 6 * (size_t)P.nb, Q = (size_t)q;
    const size_t wstride = 36 * (size_t)std::max(P.max_seg, 1);   // doubles of one queried node's W
    if ((rc = pg_upload(ctx, g->d_mq, qnode)) || (rc = reserve(ctx, g->d_mW, 8 * wstride * Q)) ||
        (rc = reserve(ctx, g->d_mblk, 8 * 72 * Q)) || (rc = reserve(ctx, g->d_mX, 8 * std::max<size_t>(nr * 6 * Q, 1))) ||
        (rc = reserve(ctx, g->d_mout, 8 * 36 * Q * Q)))
        return rc;
    const int32_t *dq = (const int32_t *)g->d_mq.p, *node_seg = (const int32_t *)g->d_node_seg.p,
                  *sep_pos = (const int32_t *)g->d_sep_pos.p;
    const PgSeg *segs = (const PgSeg *)g->d_segs.p;
    if (P.nseg > 0)
        hipLaunchKernelGGL(k_pg_marg_segment, dim3(q), dim3(64), 0, s, dq, node_seg, segs, (const double *)g->d_Cn.p,
                           (const double *)g->d_L.p, (const double *)g->d_U.p, (int)wstride,
                           (double *)g->d_mW.p, (double *)g->d_mblk.p);
    if (P.nb > 0) {
        hipLaunchKernelGGL(k_pg_marg_rhs, dim3(pg_grid(nr * 6 * Q, 256)), dim3(256), 0, s, dq, node_seg, segs, sep_pos,
                           (const double *)g->d_mblk.p, (int)q, (int)nr, (double *)g->d_mX.p);
        hipLaunchKernelGGL(k_pg_trsm_pair, dim3(q), dim3(kPgTrsmThreads), 0, s, (const double *)g->d_S.p, (int)nr,
                           (double *)g->d_mX.p);
    }
    hipLaunchKernelGGL(k_pg_marg_gather, dim3((unsigned)(Q * Q)), dim3(64), 0, s, dq, node_seg, segs, sep_pos,
                       (const double *)g->d_Y.p, (const double *)g->d_mW.p, (int)wstride, (const double *)g->d_mX.p, (int)q,
                       (int)nr,
                       (double *)g->d_mout.p);
    HIP_TRY(ctx, hipMemcpyAsync(cov, g->d_mout.p, 8 * 36 * Q * Q, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

// Sigma_rel of (from, to) and the two optimised poses
int pg_relative(icpmi_pose_graph *g, int64_t from, int64_t to, double *cov)
{
    int rc;
    if ((rc = pg_marg_state(g))) return rc;
    if (from == to) return fail(g->ctx, ICPMI_ERR_ARG, "a relative covariance needs two different poses");
    const int64_t idx[2] = {from, to};
    double joint[144];
    if ((rc = pg_marginals(g, idx, 2, joint))) return rc;
    pg_relative_covariance(g->opt.data() + 12 * from, g->opt.data() + 12 * to, joint, cov);
    return ICPMI_OK;
}

} // namespace

extern "C" {

void icpmi_pose_graph_config_default(icpmi_pose_graph_config *c)
{
    if (!c) return;
    c->odom_rotation_sigma = 0.01;       // pose_graph.hpp:25-39
    c->odom_translation_sigma = 0.05;
    c->prior_rotation_sigma = 0.001;
    c->prior_translation_sigma = 0.001;
    c->loop_rotation_sigma = 0.005;
    c->loop_translation_sigma = 0.025;
    c->max_iterations = 100;
    c->reserved = 0;
    c->relative_error_tol = 1e-5;
    c->absolute_error_tol = 1e-5;
}

int icpmi_pose_graph_create(icpmi_ctx *ctx, const icpmi_pose_graph_config *cfg, icpmi_pose_graph **out)
{
    int rc;
    if (!out) return fail(ctx, ICPMI_ERR_NULL, "out is NULL");
    *out = nullptr;
    if ((rc = check_common(ctx))) return rc;
    icpmi_pose_graph_config c;
    if (cfg) c = *cfg;
    else icpmi_pose_graph_config_default(&c);
    const double sig[6] = {c.odom_rotation_sigma, c.odom_translation_sigma, c.prior_rotation_sigma,
                           c.prior_translation_sigma, c.loop_rotation_sigma, c.loop_translation_sigma};
    for (double v : sig)
        if (!(v > 0.0) || !std::isfinite(v)) return fail(ctx, ICPMI_ERR_ARG, "sigmas must be finite and positive");
    if (c.max_iterations < 0 || !(c.relative_error_tol >= 0.0) || !(c.absolute_error_tol >= 0.0))
        return fail(ctx, ICPMI_ERR_ARG, "bad optimizer settings");
    icpmi_pose_graph *g = new icpmi_pose_graph;
    g->ctx = ctx;
    g->cfg = c;
    if (hipHostMalloc((void **)&g->h_out, 64) != hipSuccess) {
        delete g;
        return fail(ctx, ICPMI_ERR_HIP, "hipHostMalloc failed");
    }
    *out = g;
    return ICPMI_OK;
}

void icpmi_pose_graph_destroy(icpmi_pose_graph *g)
{
    if (!g) return;
    (void)hipSetDevice(g->ctx->opt.device);
    (void)hipStreamSynchronize(g->ctx->stream);
    DevBuf *bufs[] = {&g->d_fac, &g->d_init, &g->d_map, &g->d_keys, &g->d_X, &g->d_Xc, &g->d_A, &g->d_rw, &g->d_err,
                      &g->d_H, &g->d_g, &g->d_D, &g->d_gn, &g->d_Cn, &g->d_L, &g->d_U, &g->d_Y, &g->d_schur, &g->d_S,
                      &g->d_xb, &g->d_delta, &g->d_errc, &g->d_errl, &g->d_out, &g->d_status, &g->d_inc_ptr, &g->d_inc,
                      &g->d_cn_ptr, &g->d_cn, &g->d_segs, &g->d_blocks, &g->d_codes, &g->d_sep_node, &g->d_sep_segs,
                      &g->d_sep_pos, &g->d_node_seg, &g->d_rank, &g->d_wd, &g->d_slot, &g->d_infoR, &g->d_mq,
                      &g->d_mW, &g->d_mblk, &g->d_mX, &g->d_mout};
    for (DevBuf *b : bufs) release(*b);
    if (g->h_out) (void)hipHostFree(g->h_out);
    delete g;
}

int icpmi_pose_graph_add_prior(icpmi_pose_graph *g, int64_t index, const double pose[16])
{
    if (!g) return ICPMI_ERR_NULL;
    int rc;
    if ((rc = pg_check_T(g->ctx, pose))) return rc;
    if (index < 0 || index >= INT32_MAX - 1) return fail(g->ctx, ICPMI_ERR_ARG, "pose index out of range");
    const double c = g->cfg.prior_rotation_sigma, t = g->cfg.prior_translation_sigma;
    PgFactor f;
    pg_factor(f, 0, index, -1, pose, c, t);
    g->factors.push_back(f);                       // graph_->addPrior (pose_graph.cpp:72)
    g->info_slot.push_back(-1);
    g->marg_factored = false;
    if (!pg_has(g, index)) pg_set_init(g, index, f.Z);   // :75-78; optimized_ is left as it is
    return ICPMI_OK;
}

// addOdometryFactor with either noise model: `info` null, the reference's diagonal sigmas scaled by 1 + 10 fitness; else
// the 6 x 6 information matrix, factored here and refused before anything changes
static int pg_add_odometry(icpmi_pose_graph *g, int64_t from, int64_t to, const double rel[16], double fitness,
                           const double *info)
{
    int rc;
    if ((rc = pg_check_T(g->ctx, rel))) return rc;
    if (from < 0 || to < 0 || from >= INT32_MAX - 1 || to >= INT32_MAX - 1 || from == to || !std::isfinite(fitness))
        return fail(g->ctx, ICPMI_ERR_ARG, "bad odometry factor");
    const bool need = !pg_has(g, to);
    if (need && !pg_has(g, from))                  // Values::at throws in the reference (pose_graph.cpp:104)
        return fail(g->ctx, ICPMI_ERR_ARG, "pose %lld has no estimate", (long long)from);
    double R21[21];
    if (info && (rc = pg_factor_information(g->ctx, info, R21))) return rc;
    const double scale = 1.0 + fitness * 10.0;     // :88
    PgFactor f;
    pg_factor(f, 1, from, to, rel, g->cfg.odom_rotation_sigma * scale, g->cfg.odom_translation_sigma * scale);
    g->factors.push_back(f);                       // :99-101
    pg_push_slot(g, info ? R21 : nullptr);
    if (need) {                                    // :103-110: X_to = X_from * Z (Pose3::compose)
        const double *a = g->init.data() + 12 * from, *b = f.Z;
        double o[12];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
        for (int i = 0; i < 3; ++i) o[9 + i] = (a[3 * i] * b[9] + a[3 * i + 1] * b[10] + a[3 * i + 2] * b[11]) + a[9 + i];
        pg_set_init(g, to, o);
    }
    g->optimized = false;                          // :112
    g->marg_factored = false;
    return ICPMI_OK;
}

static int pg_add_loop_closure(icpmi_pose_graph *g, int64_t from, int64_t to, const double rel[16], const double *info)
{
    int rc;
    if ((rc = pg_check_T(g->ctx, rel))) return rc;
    if (from < 0 || to < 0 || from >= INT32_MAX - 1 || to >= INT32_MAX - 1 || from == to)
        return fail(g->ctx, ICPMI_ERR_ARG, "bad loop closure");
    double R21[21];
    if (info && (rc = pg_factor_information(g->ctx, info, R21))) return rc;
    PgFactor f;
    pg_factor(f, 1, from, to, rel, g->cfg.loop_rotation_sigma, g->cfg.loop_translation_sigma);
    f.reserved = 1;
    g->factors.push_back(f);                       // pose_graph.cpp:132-134
    pg_push_slot(g, info ? R21 : nullptr);
    g->num_loops++;                                // :136
    g->optimized = false;                          // :137
    g->marg_factored = false;
    return ICPMI_OK;
}

int icpmi_pose_graph_add_odometry(icpmi_pose_graph *g, int64_t from, int64_t to, const double rel[16], double fitness)
{
    if (!g) return ICPMI_ERR_NULL;
    return pg_add_odometry(g, from, to, rel, fitness, nullptr);
}

int icpmi_pose_graph_add_loop_closure(icpmi_pose_graph *g, int64_t from, int64_t to, const double rel[16])
{
    if (!g) return ICPMI_ERR_NULL;
    return pg_add_loop_closure(g, from, to, rel, nullptr);
}

int icpmi_pose_graph_add_odometry_information(icpmi_pose_graph *g, int64_t from, int64_t to, const double rel[16],
                                              const double info[36])
{
    if (!g) return ICPMI_ERR_NULL;
    if (!info) return fail(g->ctx, ICPMI_ERR_NULL, "info is NULL");
    return pg_add_odometry(g, from, to, rel, 0.0, info);
}

int icpmi_pose_graph_add_loop_closure_information(icpmi_pose_graph *g, int64_t from, int64_t to, const double rel[16],
                                                  const double info[36])
{
    if (!g) return ICPMI_ERR_NULL;
    if (!info) return fail(g->ctx, ICPMI_ERR_NULL, "info is NULL");
    return pg_add_loop_closure(g, from, to, rel, info);
}

int icpmi_information_from_icp(const double JtJ[36], const double T[16], double sigma, double floor_rotation_sigma,
                               double floor_translation_sigma, double info_out[36])
{
    if (!JtJ || !T || !info_out) return ICPMI_ERR_NULL;
    double out[36];
    if (!pg_information_from_icp(JtJ, T, sigma, floor_rotation_sigma, floor_translation_sigma, out)) return ICPMI_ERR_ARG;
    memcpy(info_out, out, sizeof(out));
    return ICPMI_OK;
}

// grow keeping the first `used` bytes (the incremental uploads)
static int pg_reserve_keep(icpmi_ctx *ctx, DevBuf &b, size_t used, size_t bytes)
{
    if (bytes <= b.cap) return ICPMI_OK;
    DevBuf nb;
    HIP_TRY(ctx, reserve_raw(nb, std::max(bytes, 2 * b.cap)));
    if (used) HIP_TRY(ctx, hipMemcpyAsync(nb.p, b.p, used, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    release(b);
    b = nb;
    return ICPMI_OK;
}

int icpmi_pose_graph_optimize(icpmi_pose_graph *g, icpmi_pose_graph_info *info, double *history, int32_t history_cap)
{
    if (!g) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = g->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    const icpmi_pose_graph_config &c = g->cfg;
    if (history && history_cap < c.max_iterations + 1)
        return fail(ctx, ICPMI_ERR_CAPACITY, "history needs max_iterations + 1 entries");
    icpmi_pose_graph_info st;
    memset(&st, 0, sizeof(st));
    if (info) *info = st;
    if (g->num_poses == 0) return ICPMI_OK;                 // pose_graph.cpp:148-150: false, nothing changes
    for (const PgFactor &f : g->factors)
        if (!pg_has(g, f.i) || (f.kind == 1 && !pg_has(g, f.j)))
            return fail(ctx, ICPMI_ERR_ARG, "a factor names pose %lld, which has no estimate",
                        (long long)(pg_has(g, f.i) ? f.j : f.i));   // the reference's catch (:166-169)
    hipStream_t s = ctx->stream;
    g->values_on_device = false;
    g->marg_factored = false;
    // only what was added since the last call goes up: the new factors and the new estimates
    const size_t F = g->factors.size();
    if ((rc = pg_reserve_keep(ctx, g->d_fac, sizeof(PgFactor) * g->uploaded_factors, sizeof(PgFactor) * F))) return rc;
    if (F > g->uploaded_factors)
        HIP_TRY(ctx, hipMemcpyAsync((PgFactor *)g->d_fac.p + g->uploaded_factors, g->factors.data() + g->uploaded_factors,
                                    sizeof(PgFactor) * (F - g->uploaded_factors), hipMemcpyHostToDevice, s));
    g->uploaded_factors = F;
    if (!g->info_R.empty()) {   // the slots of all factors and the new R go up from the first information factor on
        const size_t nR = g->info_R.size();
        if ((rc = pg_reserve_keep(ctx, g->d_slot, sizeof(int32_t) * g->uploaded_slots, sizeof(int32_t) * F)) ||
            (rc = pg_reserve_keep(ctx, g->d_infoR, sizeof(double) * g->uploaded_R, sizeof(double) * nR)))
            return rc;
        if (F > g->uploaded_slots)
            HIP_TRY(ctx, hipMemcpyAsync((int32_t *)g->d_slot.p + g->uploaded_slots, g->info_slot.data() + g->uploaded_slots,
                                        sizeof(int32_t) * (F - g->uploaded_slots), hipMemcpyHostToDevice, s));
        if (nR > g->uploaded_R)
            HIP_TRY(ctx, hipMemcpyAsync((double *)g->d_infoR.p + g->uploaded_R, g->info_R.data() + g->uploaded_R,
                                        sizeof(double) * (nR - g->uploaded_R), hipMemcpyHostToDevice, s));
        g->uploaded_slots = F;
        g->uploaded_R = nR;
    }
    const size_t init_used = g->d_init.cap / 96 * 96;
    if ((rc = pg_reserve_keep(ctx, g->d_init, init_used, 96 * (size_t)g->num_poses))) return rc;
    if (g->init_dirty_hi > g->init_dirty_lo) {
        const int64_t lo = g->init_dirty_lo, hi = g->init_dirty_hi;
        HIP_TRY(ctx, hipMemcpyAsync((double *)g->d_init.p + 12 * lo, g->init.data() + 12 * lo, 96 * (size_t)(hi - lo),
                                    hipMemcpyHostToDevice, s));
        g->init_dirty_lo = INT64_MAX;
        g->init_dirty_hi = 0;
    }
    PgPlan P;
    if ((rc = pg_plan(g, P))) return rc;
    PgLin lin{(double *)g->d_A.p, (double *)g->d_rw.p, (double *)g->d_err.p, (double *)g->d_H.p, (double *)g->d_g.p};
    // optimize() always starts from the initial estimates (pose_graph.cpp:153: the optimizer gets *initial_estimates_)
    hipLaunchKernelGGL(k_pg_gather, dim3(pg_grid(12 * (size_t)P.n, 256)), dim3(256), 0, s, (const double *)g->d_init.p,
                       (const int32_t *)g->d_keys.p, P.n, (double *)g->d_X.p);

    // ---- LevenbergMarquardtParams defaults; the caller's maxIterations / relativeErrorTol / absoluteErrorTol
    double lam = 1e-5;                                    // lambdaInitial
    const double lam_factor = 10.0, lam_lower = 0.0, lam_upper = 1e5, min_fidelity = 1e-3;
    const double rel_tol = c.relative_error_tol, abs_tol = c.absolute_error_tol, err_tol = 0.0;   // errorTol 0
    double error, lin0 = 0.0;
    if ((rc = pg_linearize(g, P, lin, &error, &lin0))) return rc;
    st.initial_error = error;
    int nh = 0;
    if (history) history[nh] = error;
    ++nh;
    bool linearized = true;                               // lin holds the linearisation at X
    // NonlinearOptimizer::defaultOptimize: nothing to do when the error is already <= errorTol or no iteration allowed
    if (error <= err_tol) st.stop_reason = ICPMI_PG_STOP_ZERO_ERROR;
    else if (c.max_iterations <= 0) st.stop_reason = ICPMI_PG_STOP_MAX_ITERATIONS;
    while (st.stop_reason == ICPMI_PG_STOP_NONE) {
        const double current = error;
        // LevenbergMarquardtOptimizer::iterate: linearise once, then tryLambda until it returns true
        if (!linearized && (rc = pg_linearize(g, P, lin, nullptr, &lin0))) return rc;
        // linear.error(VectorValues::Zero) = 0.5 sum ||rw||^2: the error itself, except under a loss (rho against w d^2)
        const double old_lin = P.loss ? lin0 : current;
        bool stepped = false;
        int inner_stop = ICPMI_PG_STOP_NONE;
        double new_err = 0.0;
        for (;;) {
            st.inner_iterations++;
            // tryLambda: buildDampedSystem adds lambda I (diagonalDamping off); solve; a Cholesky that meets a
            // non-positive pivot is an unsolved system (IndeterminantLinearSystemException)
            double out[3];
            if ((rc = pg_trial(g, P, lin, lam, out))) return rc;
            const bool solved = out[2] == 0.0 && std::isfinite(out[1]);
            bool step_ok = false, stop_search = false;
            if (solved) {
                const double lin_change = old_lin - out[1];
                if (lin_change >= 0.0) {                  // tryLambda: the step is valid
                    new_err = out[0];
                    const double cost_change = current - new_err;
                    if (lin_change > std::numeric_limits<double>::epsilon() * old_lin)
                        step_ok = cost_change / lin_change > min_fidelity;   // tryLambda: modelFidelity
                    else
                        step_ok = true;                   // linearised change ~ 0
                    // tryLambda: stop searching lambda once |costChange| < relativeErrorTol * error
                    stop_search = std::fabs(cost_change) < rel_tol * current;
                }
            }
            if (step_ok) {
                lam = std::max(lam_lower, lam / lam_factor);   // State::decreaseLambda (useFixedLambdaFactor)
                std::swap(g->d_X, g->d_Xc);
                error = new_err;
                st.iterations++;
                stepped = true;
                break;
            }
            if (stop_search) {
                inner_stop = ICPMI_PG_STOP_SMALL_COST_CHANGE;
                break;
            }
            lam *= lam_factor;                            // State::increaseLambda
            if (lam >= lam_upper) {                       // tryLambda: lambda too big, give up
                inner_stop = ICPMI_PG_STOP_LAMBDA_BOUND;
                break;
            }
        }
        linearized = !stepped;
        if (history) history[nh] = error;
        ++nh;
        // defaultOptimize's loop condition: iterations < maxIterations && !checkConvergence(...) && isfinite(error)
        if (!stepped) st.stop_reason = inner_stop;        // the error did not move: checkConvergence holds
        else if (st.iterations >= c.max_iterations) st.stop_reason = ICPMI_PG_STOP_MAX_ITERATIONS;
        else if (!std::isfinite(current)) st.stop_reason = ICPMI_PG_STOP_NOT_FINITE;
        else {
            const double abs_dec = current - error, rel_dec = abs_dec / current;   // checkConvergence
            if (error <= err_tol) st.stop_reason = ICPMI_PG_STOP_ZERO_ERROR;
            else if (rel_tol != 0.0 && rel_dec <= rel_tol) st.stop_reason = ICPMI_PG_STOP_RELATIVE;
            else if (abs_dec <= abs_tol) st.stop_reason = ICPMI_PG_STOP_ABSOLUTE;
        }
    }
    // the optimised values back to the host, by pose index
    std::vector<double> X(12 * (size_t)P.n);
    HIP_TRY(ctx, hipMemcpyAsync(X.data(), g->d_X.p, sizeof(double) * X.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipGetLastError());
    g->opt.assign(12 * (size_t)g->num_poses, 0.0);
    for (int k = 0; k < P.n; ++k) std::copy(X.begin() + 12 * k, X.begin() + 12 * (k + 1), g->opt.begin() + 12 * (size_t)P.keys[k]);
    g->optimized = true;                                  // pose_graph.cpp:160-162
    g->values_on_device = true;
    g->opt_factors = P.F;
    g->opt_loops = P.nloops;
    g->plan = std::move(P);
    st.optimized = 1;
    st.final_error = error;
    st.final_lambda = lam;
    st.history_len = nh;
    g->last = st;
    if (info) *info = st;
    return ICPMI_OK;
}

int icpmi_pose_graph_set_loop_loss(icpmi_pose_graph *g, int32_t kind, double scale)
{
    if (!g) return ICPMI_ERR_NULL;
    if (kind < ICPMI_PG_LOSS_NONE || kind > ICPMI_PG_LOSS_GEMAN_MCCLURE)
        return fail(g->ctx, ICPMI_ERR_ARG, "loss kind %d is not one of ICPMI_PG_LOSS_*", (int)kind);
    if (kind == ICPMI_PG_LOSS_NONE) scale = 0.0;
    else if (!std::isfinite(scale) || !(scale > 0.0))
        return fail(g->ctx, ICPMI_ERR_ARG, "the loss scale must be finite and positive");
    g->marg_factored = false;
    if (kind == g->loss_kind && scale == g->loss_scale) return ICPMI_OK;
    g->loss_kind = kind;
    g->loss_scale = scale;
    g->optimized = false;                          // as adding a factor does
    return ICPMI_OK;
}

int icpmi_pose_graph_loop_loss(const icpmi_pose_graph *g, int32_t *kind, double *scale)
{
    if (!g) return ICPMI_ERR_NULL;
    if (kind) *kind = g->loss_kind;
    if (scale) *scale = g->loss_scale;
    return ICPMI_OK;
}

int icpmi_pose_graph_loop_weights(icpmi_pose_graph *g, double *weights, double *distances, int64_t cap, int64_t *n_out)
{
    if (!g) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = g->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (n_out) *n_out = g->num_loops;
    if (!g->optimized || !g->values_on_device || g->opt_loops != g->num_loops)
        return fail(ctx, ICPMI_ERR_ARG, "loop weights need the optimised state of the last optimize()");
    if (!weights && !distances) return ICPMI_OK;
    const int64_t nl = g->num_loops;
    if (cap < nl) return fail(ctx, ICPMI_ERR_CAPACITY, "%lld loop closures need room", (long long)nl);
    if (nl == 0) return ICPMI_OK;
    hipStream_t s = ctx->stream;
    const int F = g->opt_factors;
    if (!g->info_R.empty())   // (the optimised state holds: every factor's slot went up with that optimize())
        hipLaunchKernelGGL(k_pg_loop_weights_info, dim3(pg_grid(F, 128)), dim3(128), 0, s, (const PgFactor *)g->d_fac.p,
                           (const int32_t *)g->d_slot.p, (const double *)g->d_infoR.p, (const int32_t *)g->d_map.p,
                           (const int32_t *)g->d_rank.p, F, (const double *)g->d_X.p, (int)g->loss_kind, g->loss_scale,
                           (double *)g->d_wd.p);
    else
        hipLaunchKernelGGL(k_pg_loop_weights, dim3(pg_grid(F, 128)), dim3(128), 0, s, (const PgFactor *)g->d_fac.p,
                           (const int32_t *)g->d_map.p, (const int32_t *)g->d_rank.p, F, (const double *)g->d_X.p,
                           (int)g->loss_kind, g->loss_scale, (double *)g->d_wd.p);
    std::vector<double> wd(2 * (size_t)nl);
    HIP_TRY(ctx, hipMemcpyAsync(wd.data(), g->d_wd.p, sizeof(double) * wd.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipGetLastError());
    for (int64_t k = 0; k < nl; ++k) {
        if (weights) weights[k] = wd[2 * k];
        if (distances) distances[k] = wd[2 * k + 1];
    }
    return ICPMI_OK;
}

int icpmi_pose_graph_marginals(icpmi_pose_graph *g, const int64_t *indices, int32_t q, double *cov)
{
    if (!g) return ICPMI_ERR_NULL;
    int rc;
    if ((rc = check_common(g->ctx))) return rc;
    if (!indices || !cov) return fail(g->ctx, ICPMI_ERR_NULL, "indices or cov is NULL");
    return pg_marginals(g, indices, q, cov);
}

int icpmi_pose_graph_relative_covariance(icpmi_pose_graph *g, int64_t from, int64_t to, double cov[36])
{
    if (!g) return ICPMI_ERR_NULL;
    int rc;
    if ((rc = check_common(g->ctx))) return rc;
    if (!cov) return fail(g->ctx, ICPMI_ERR_NULL, "cov is NULL");
    return pg_relative(g, from, to, cov);
}

int icpmi_pose_graph_closure_distance(icpmi_pose_graph *g, int64_t from, int64_t to, const double rel[16],
                                      const double edge_cov[36], double *d2)
{
    if (!g) return ICPMI_ERR_NULL;
    int rc;
    if ((rc = check_common(g->ctx))) return rc;
    if (!edge_cov || !d2) return fail(g->ctx, ICPMI_ERR_NULL, "edge_cov or d2 is NULL");
    if ((rc = pg_check_T(g->ctx, rel))) return rc;
    double cov[36], Z[12];
    if ((rc = pg_relative(g, from, to, cov))) return rc;
    pg_to12(rel, Z);
    if (!pg_closure_distance(g->opt.data() + 12 * from, g->opt.data() + 12 * to, Z, cov, edge_cov, d2))
        return fail(g->ctx, ICPMI_ERR_ARG, "the relative covariance plus the edge covariance is not positive definite");
    return ICPMI_OK;
}

int icpmi_pose_graph_pose(icpmi_pose_graph *g, int64_t index, double pose[16])
{
    if (!g) return ICPMI_ERR_NULL;
    if (!pose) return fail(g->ctx, ICPMI_ERR_NULL, "pose is NULL");
    if (!pg_has(g, index)) return fail(g->ctx, ICPMI_ERR_ARG, "Pose index %lld not found", (long long)index);   // :181-183
    pg_to16((g->optimized ? g->opt.data() : g->init.data()) + 12 * index, pose);   // :180
    return ICPMI_OK;
}

int icpmi_pose_graph_poses(icpmi_pose_graph *g, double *poses, int64_t cap, int64_t *n_out, int64_t *indices)
{
    if (!g) return ICPMI_ERR_NULL;
    int64_t cnt = 0;
    for (int64_t k = 0; k < g->num_poses; ++k) cnt += pg_has(g, k);
    if (n_out) *n_out = cnt;
    if (!poses && !indices) return ICPMI_OK;
    if (cap < cnt) return fail(g->ctx, ICPMI_ERR_CAPACITY, "%lld poses need room", (long long)cnt);
    const double *src = g->optimized ? g->opt.data() : g->init.data();
    int64_t o = 0;
    for (int64_t k = 0; k < g->num_poses; ++k)      // pose_graph.cpp:194-198: 0 .. num_poses_-1, gaps skipped
        if (pg_has(g, k)) {
            if (poses) pg_to16(src + 12 * k, poses + 16 * o);
            if (indices) indices[o] = k;
            ++o;
        }
    return ICPMI_OK;
}

int icpmi_pose_graph_size(const icpmi_pose_graph *g, int64_t *num_poses, int64_t *num_loop_closures,
                          icpmi_pose_graph_info *last)
{
    if (!g) return ICPMI_ERR_NULL;
    if (num_poses) *num_poses = g->num_poses;                 // pose_graph.hpp:117
    if (num_loop_closures) *num_loop_closures = g->num_loops; // :122
    if (last) *last = g->last;                                // :127-128 (final error, iterations)
    return ICPMI_OK;
}

} // extern "C"

// ======================================================================================================================
// Ground segmentation of a scan in its sensor frame (ground.h).

static_assert(kGroundMaxBins == ICPMI_GROUND_MAX_BINS && kGroundObstacle == ICPMI_GROUND_OBSTACLE &&
                  kGroundGround == ICPMI_GROUND_GROUND && kGroundIgnored == ICPMI_GROUND_IGNORED,
              "the header states these");

namespace {

int ground_check(icpmi_ctx *ctx, const icpmi_ground_config *c)
{
    if (!c) return fail(ctx, ICPMI_ERR_NULL, "the ground config is NULL");
    for (double v : {c->min_range, c->max_range, c->sensor_height, c->max_slope, c->step_tol, c->height_tol, c->clear_min, c->clear_max})
        if (!std::isfinite(v)) return fail(ctx, ICPMI_ERR_ARG, "a ground config field is not finite");
    if (c->n_rings < 1 || c->n_sectors < 1) return fail(ctx, ICPMI_ERR_ARG, "n_rings and n_sectors must be at least 1");
    if ((int64_t)c->n_rings * (int64_t)c->n_sectors > kGroundMaxBins)
        return fail(ctx, ICPMI_ERR_ARG, "n_rings * n_sectors must be at most %d", kGroundMaxBins);
    if (c->min_range < 0.0 || !(c->max_range > c->min_range)) return fail(ctx, ICPMI_ERR_ARG, "0 <= min_range < max_range is required");
    if (c->max_slope < 0.0 || c->step_tol < 0.0 || c->height_tol < 0.0)
        return fail(ctx, ICPMI_ERR_ARG, "max_slope, step_tol and height_tol must not be negative");
    if (c->clear_max < c->clear_min) return fail(ctx, ICPMI_ERR_ARG, "clear_max < clear_min");
    return ICPMI_OK;
}

// Queue k_ground_label for `scans` scans of `store` (checked config).
int ground_queue(icpmi_ctx *ctx, const icpmi_ground_config *c, const double *store, const GroundFrame *frames_d, int64_t scans,
                 uint8_t *labels, double *height, double *ground_z, GroundCounts *counts)
{
    const GroundParams p{c->n_rings,  c->n_sectors,   c->min_range, c->max_range, c->sensor_height,
                         c->max_slope, c->step_tol, c->height_tol, c->clear_min, c->clear_max};
    const size_t lds = sizeof(unsigned long long) * (size_t)c->n_rings * (size_t)c->n_sectors;
    if (lds > 64 * 1024) // dynamic LDS past 64 KiB has to be allowed first
        HIP_TRY(ctx, hipFuncSetAttribute((const void *)k_ground_label, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)sizeof(unsigned long long) * kGroundMaxBins));
    hipLaunchKernelGGL(k_ground_label, dim3((unsigned)scans), dim3(kGroundThreads), lds, ctx->stream, store, frames_d, p, labels,
                       height, ground_z, counts);
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

int ground_segment(icpmi_ctx *ctx, const double *xyz, bool on_device, int64_t n, const icpmi_ground_config *cfg, uint8_t *labels,
                   double *height, double *ground_z, icpmi_ground_info *info)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if ((rc = ground_check(ctx, cfg))) return rc;
    if (n < 0 || n > 700000000) return fail(ctx, ICPMI_ERR_ARG, "n out of range");
    if (n > 0 && (!xyz || !labels)) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    Range range("icpmi:ground_segment");
    hipStream_t s = ctx->stream;
    const size_t un = (size_t)n, bins = (size_t)cfg->n_rings * (size_t)cfg->n_sectors;
    // the launch's outputs in one buffer: the frame table, the counts, ground_z, height, labels
    const size_t o_counts = sizeof(GroundFrame), o_gz = o_counts + sizeof(GroundCounts), o_h = o_gz + sizeof(double) * bins,
                 o_lab = o_h + sizeof(double) * un;
    if ((rc = reserve(ctx, ctx->stage_b, o_lab + un))) return rc;
    char *out = (char *)ctx->stage_b.p;
    const double *rows = xyz;
    if (!on_device && n > 0) {
        if ((rc = reserve(ctx, ctx->stage_a, sizeof(double) * 3 * un))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_a.p, xyz, sizeof(double) * 3 * un, hipMemcpyHostToDevice, s));
        rows = (const double *)ctx->stage_a.p;
    }
    const GroundFrame f{0, (int32_t)n, 0};
    GroundCounts cnt{};
    HIP_TRY(ctx, hipMemcpyAsync(out, &f, sizeof(f), hipMemcpyHostToDevice, s));
    if ((rc = ground_queue(ctx, cfg, rows, (const GroundFrame *)out, 1, (uint8_t *)(out + o_lab), height ? (double *)(out + o_h) : nullptr,
                           ground_z ? (double *)(out + o_gz) : nullptr, (GroundCounts *)(out + o_counts))))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(&cnt, out + o_counts, sizeof(cnt), hipMemcpyDeviceToHost, s));
    if (ground_z) HIP_TRY(ctx, hipMemcpyAsync(ground_z, out + o_gz, sizeof(double) * bins, hipMemcpyDeviceToHost, s));
    if (height && n > 0) HIP_TRY(ctx, hipMemcpyAsync(height, out + o_h, sizeof(double) * un, hipMemcpyDeviceToHost, s));
    if (n > 0) HIP_TRY(ctx, hipMemcpyAsync(labels, out + o_lab, un, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s)); // the call's one wait
    HIP_TRY(ctx, hipGetLastError());
    if (info) *info = icpmi_ground_info{(int64_t)cnt.n_ground, (int64_t)cnt.n_obstacle, (int64_t)cnt.n_ignored, (int64_t)cnt.bins_accepted};
    return ICPMI_OK;
}

} // namespace

extern "C" {

void icpmi_ground_config_default(icpmi_ground_config *cfg)
{
    if (!cfg) return;
    *cfg = icpmi_ground_config{80, 180, 0.5, 80.5, 1.73, 0.15, 0.1, 0.2, 0.3, 2.0};
}

int icpmi_ground_segment(icpmi_ctx *ctx, const double *xyz, int64_t n, const icpmi_ground_config *cfg, uint8_t *labels,
                         double *height, double *ground_z, icpmi_ground_info *info)
{
    return ground_segment(ctx, xyz, false, n, cfg, labels, height, ground_z, info);
}

int icpmi_ground_segment_device(icpmi_ctx *ctx, const double *d_xyz, int64_t n, const icpmi_ground_config *cfg, uint8_t *labels,
                                double *height, double *ground_z, icpmi_ground_info *info)
{
    return ground_segment(ctx, d_xyz, true, n, cfg, labels, height, ground_z, info);
}

} // extern "C"

// ======================================================================================================================
// Motion compensation of a scan in its sensor frame (deskew.h, deskew_host.h).

static_assert(kDeskewTimes == ICPMI_DESKEW_TIMES && kDeskewAzimuth == ICPMI_DESKEW_AZIMUTH, "the header states these");

namespace {

int deskew_check_config(icpmi_ctx *ctx, const icpmi_deskew_config *c)
{
    if (!c) return fail(ctx, ICPMI_ERR_NULL, "the deskew config is NULL");
    const DeskewRefusal r = deskew_check(c->twist, c->t_ref, c->time_source, c->direction, c->azimuth_start);
    if (r != kDeskewOk) return fail(ctx, ICPMI_ERR_ARG, "%s", deskew_refusal_text(r));
    return ICPMI_OK;
}

// Queue k_deskew for n > 0 rows on the context's stream (checked config; d_out may be d_xyz).
int deskew_queue(icpmi_ctx *ctx, const icpmi_deskew_config *c, const double *d_xyz, const double *d_times, int64_t n, double *d_out)
{
    const DeskewConstants k = deskew_constants(c->twist, c->t_ref, c->time_source, c->direction, c->azimuth_start);
    const unsigned blocks = (unsigned)std::min<int64_t>(kDeskewMaxBlocks, (n + kDeskewThreads - 1) / kDeskewThreads);
    hipLaunchKernelGGL(k_deskew, dim3(blocks), dim3(kDeskewThreads), 0, ctx->stream, d_xyz, d_times, d_out, (size_t)n, k);
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

int deskew_args(icpmi_ctx *ctx, const double *xyz, const double *times, int64_t n, const icpmi_deskew_config *cfg, double *out)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if ((rc = deskew_check_config(ctx, cfg))) return rc;
    if (n < 0 || n > 700000000) return fail(ctx, ICPMI_ERR_ARG, "n out of range");
    if (n > 0 && (!xyz || !out)) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (n > 0 && cfg->time_source == ICPMI_DESKEW_TIMES && !times)
        return fail(ctx, ICPMI_ERR_NULL, "ICPMI_DESKEW_TIMES without times");
    return ICPMI_OK;
}

} // namespace

extern "C" {

void icpmi_deskew_config_default(icpmi_deskew_config *cfg)
{
    if (!cfg) return;
    *cfg = icpmi_deskew_config{};
    cfg->t_ref = 0.5;
    cfg->time_source = ICPMI_DESKEW_TIMES;
    cfg->direction = 1;
    cfg->azimuth_start = -3.14159265358979323846;
}

int icpmi_deskew_twist(const double delta[16], double twist[6])
{
    if (!delta || !twist) return fail(nullptr, ICPMI_ERR_NULL, "null argument");
    if (!deskew_twist(delta, twist)) return fail(nullptr, ICPMI_ERR_ARG, "a pose entry is not finite");
    return ICPMI_OK;
}

int icpmi_deskew_device(icpmi_ctx *ctx, const double *d_xyz, const double *d_times, int64_t n, const icpmi_deskew_config *cfg,
                        double *d_out_xyz)
{
    int rc;
    if ((rc = deskew_args(ctx, d_xyz, d_times, n, cfg, d_out_xyz))) return rc;
    if (n == 0) return ICPMI_OK;
    Range range("icpmi:deskew");
    return deskew_queue(ctx, cfg, d_xyz, d_times, n, d_out_xyz);
}

int icpmi_deskew(icpmi_ctx *ctx, const double *xyz, const double *times, int64_t n, const icpmi_deskew_config *cfg, double *out_xyz)
{
    int rc;
    if ((rc = deskew_args(ctx, xyz, times, n, cfg, out_xyz))) return rc;
    if (n == 0) return ICPMI_OK;
    Range range("icpmi:deskew");
    hipStream_t s = ctx->stream;
    const size_t un = (size_t)n;
    const bool with_times = cfg->time_source == ICPMI_DESKEW_TIMES;
    if ((rc = reserve(ctx, ctx->stage_a, sizeof(double) * 3 * un))) return rc;
    if (with_times && (rc = reserve(ctx, ctx->deskew_times, sizeof(double) * un))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_a.p, xyz, sizeof(double) * 3 * un, hipMemcpyHostToDevice, s));
    if (with_times) HIP_TRY(ctx, hipMemcpyAsync(ctx->deskew_times.p, times, sizeof(double) * un, hipMemcpyHostToDevice, s));
    if ((rc = deskew_queue(ctx, cfg, (const double *)ctx->stage_a.p, with_times ? (const double *)ctx->deskew_times.p : nullptr, n,
                           (double *)ctx->stage_a.p)))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_xyz, ctx->stage_a.p, sizeof(double) * 3 * un, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s)); // the call's one wait
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

int icpmi_stream_set_deskew(icpmi_ctx *ctx, const icpmi_deskew_config *cfg)
{
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!cfg) {
        ctx->stream_deskew_on = false;
        return ICPMI_OK;
    }
    if ((rc = deskew_check_config(ctx, cfg))) return rc;
    if (cfg->time_source != ICPMI_DESKEW_AZIMUTH)
        return fail(ctx, ICPMI_ERR_ARG, "the stream has no times: its deskew takes ICPMI_DESKEW_AZIMUTH");
    ctx->stream_deskew = *cfg;
    ctx->stream_deskew_on = true;
    return ICPMI_OK;
}

} // extern "C"

// ======================================================================================================================
// Global map (slam_node.cpp:187-238): the node's kept scans (downsampled_clouds_) in one device arena, and the world
// points, cell set and published map of any prefix of them from one launch of k_map_world (global_map.h).

// What a map handle remembers between icpmi_map_live_update calls: the plane and its box, the running bounds, and the
// grid and poses the frames [0, n_cast) were cast with.
struct LiveCounts {
    bool valid = false;                  // false: the next update rebuilds (nothing cast yet, cleared, or a HIP failure)
    bool windows_clean = false;          // d_windows is all zeros
    icpmi_grid_config grid{};
    int R = 0;
    int64_t n_cast = 0;
    std::vector<double> poses;           // 16 doubles per cast frame
    int64_t span[4] = {INT64_MAX, INT64_MAX, INT64_MIN, INT64_MIN};   // the sensor cells of the cast frames that hold rows
    LiveBox box;                         // the plane's cells (w == 0: no plane)
    CountBounds bounds{INT32_MAX, INT32_MAX, -1, -1, 0, 0, 0, 0};     // the host's copy after the last update
    DevBuf d_plane, d_bounds, d_windows; // one word per cell; CountBounds; k_live_carve's pair of windows
    DevBuf d_out;                        // icpmi_map_live_counts: hits, misses, probability
    icpmi_live_info info{};              // the last successful update's (all zeros before the first)
};

struct icpmi_map {
    icpmi_ctx *ctx = nullptr;
    DevBuf d_rows;                       // the store: every frame's rows, frame after frame (N x 3 fp64)
    DevBuf d_tiles;                      // the tile table (MapTile), uploaded as it grows
    DevBuf d_poses, d_world;             // a call's poses (16 doubles per frame), its world points
    std::vector<int64_t> row0{0};        // per frame its first row in the store; row0[frames] = rows
    std::vector<int64_t> tile0{0};       // per frame its first tile; tile0[frames] = tiles
    std::vector<MapTile> tiles;
    size_t uploaded_tiles = 0;           // tiles already in d_tiles
    DevBuf d_ray_frames, d_ray_planes;   // icpmi_map_raycast: the frame table; the carved and occupied planes, RayBounds
    DevBuf d_raster, d_raster_next;      // the last successful raster; the one a call is building
    icpmi_raster_info raster{};          // the last successful raster's (all zeros before the first)
    DevBuf d_count_plane, d_count_scratch; // icpmi_map_raycast_counts: the count plane and CountBounds; the windows past LDS
    DevBuf d_counts, d_counts_next;      // the last successful counts (hits, misses, probability); those a call is building
    icpmi_counts_info counts{};          // the last successful counts' (all zeros before the first)
    LiveCounts live;                     // icpmi_map_live_update: the counts that persist (live_counts.h)
    // icpmi_map_set_ground (ground.h): while ground_on, a frame's hits are its OBSTACLE rows
    bool ground_on = false;
    icpmi_ground_config ground{};
    int64_t ground_frames = 0;           // frames [0, ground_frames) are labelled
    std::vector<int32_t> ground_hits;    // per labelled frame its OBSTACLE rows
    DevBuf d_labels, d_ground_tab;       // one byte per store row; a labelling launch's frame table and counts
    // icpmi_map_world_static / icpmi_map_finish_static (static_map.h): the labels against the live counts
    DevBuf d_static_labels, d_static_tab; // one byte per store row; per tile its kept rows, their exclusive sums, StaticTotals
    int64_t static_frames = -1;          // frames [0, static_frames) hold the labels of the last call that formed them (-1: none)
};

namespace {

constexpr int64_t kMapMaxRows = 700000000; // the library's per-call limit

int64_t map_frames(const icpmi_map *m) { return (int64_t)m->row0.size() - 1; }

// downsampled_clouds_.push_back (slam_node.cpp:71,123): n rows from `src` (host or device memory, `kind`) behind the
// store's rows.  The arena grows geometrically by a device copy; the old one is freed after the call's one wait.  On
// any error the store is as it was.
int map_append(icpmi_map *m, const void *src, int64_t n, hipMemcpyKind kind)
{
    icpmi_ctx *ctx = m->ctx;
    const int64_t have = m->row0.back();
    if (n < 0 || n > kMapMaxRows - have)
        return fail(ctx, ICPMI_ERR_ARG, "the store holds %lld rows; %lld more would pass the limit of %lld", (long long)have,
                    (long long)n, (long long)kMapMaxRows);
    if (map_frames(m) >= INT32_MAX) return fail(ctx, ICPMI_ERR_ARG, "too many frames");
    hipStream_t s = ctx->stream;
    const size_t used = sizeof(double) * 3 * (size_t)have, need = sizeof(double) * 3 * (size_t)(have + n);
    DevBuf grown; // the new arena, if the store has to grow
    auto drop = [&](hipError_t e) {
        release(grown);
        return fail(ctx, ICPMI_ERR_HIP, "global map store: %s", hipGetErrorString(e));
    };
    hipError_t e = hipSuccess;
    DevBuf &dst = need > m->d_rows.cap ? grown : m->d_rows;
    if (&dst == &grown) {
        if ((e = reserve_raw(grown, std::max(need, 2 * m->d_rows.cap))) != hipSuccess) return drop(e);
        if (used && (e = hipMemcpyAsync(grown.p, m->d_rows.p, used, hipMemcpyDeviceToDevice, s)) != hipSuccess) return drop(e);
    }
    if (n && (e = hipMemcpyAsync((char *)dst.p + used, src, need - used, kind, s)) != hipSuccess) return drop(e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return drop(e); // the call's one wait
    if (&dst == &grown) {
        release(m->d_rows);
        m->d_rows = grown;
    }
    const int32_t f = (int32_t)map_frames(m);
    for (int64_t r = 0; r < n; r += kMapTileRows)
        m->tiles.push_back(MapTile{have + r, f, (int32_t)std::min<int64_t>(kMapTileRows, n - r)});
    m->row0.push_back(have + n);
    m->tile0.push_back((int64_t)m->tiles.size());
    return ICPMI_OK;
}

// The frames a call uses: [0, min(frames, n_poses)) (slam_node.cpp:190,201,225: i < downsampled_clouds_.size() &&
// i < poses_.size()).  The poses they use must be finite; map_check_poses is the two steps over every used frame.
int map_check_count(icpmi_map *m, const double *poses, int64_t n_poses, int64_t *last)
{
    icpmi_ctx *ctx = m->ctx;
    if (n_poses < 0) return fail(ctx, ICPMI_ERR_ARG, "n_poses < 0");
    if (!poses && n_poses > 0) return fail(ctx, ICPMI_ERR_NULL, "poses is NULL");
    *last = std::min(map_frames(m), n_poses);
    return ICPMI_OK;
}

int map_check_finite(icpmi_map *m, const double *poses, int64_t first, int64_t last)
{
    for (int64_t i = 16 * first; i < 16 * last; ++i)
        if (!std::isfinite(poses[i])) return fail(m->ctx, ICPMI_ERR_ARG, "pose %lld has a non-finite entry", (long long)(i / 16));
    return ICPMI_OK;
}

int map_check_poses(icpmi_map *m, const double *poses, int64_t n_poses, int64_t *last)
{
    int rc;
    if ((rc = map_check_count(m, poses, n_poses, last))) return rc;
    return map_check_finite(m, poses, 0, *last);
}

// Queue, for frames [first, last) (first < last): the tile table's new entries and the frames' poses (into d_poses,
// frame first's at its start).
int map_queue_tables(icpmi_map *m, const double *poses, int64_t first, int64_t last)
{
    icpmi_ctx *ctx = m->ctx;
    hipStream_t s = ctx->stream;
    int rc;
    const size_t T = m->tiles.size();
    if (sizeof(MapTile) * T > m->d_tiles.cap) { // grows geometrically: the whole table goes up again
        release(m->d_tiles);
        m->uploaded_tiles = 0;
        if ((rc = reserve(ctx, m->d_tiles, sizeof(MapTile) * 2 * T))) return rc;
    }
    if (T > m->uploaded_tiles)
        HIP_TRY(ctx, hipMemcpyAsync((MapTile *)m->d_tiles.p + m->uploaded_tiles, m->tiles.data() + m->uploaded_tiles,
                                    sizeof(MapTile) * (T - m->uploaded_tiles), hipMemcpyHostToDevice, s));
    m->uploaded_tiles = T;
    const size_t pose_bytes = sizeof(double) * 16 * (size_t)(last - first);
    if ((rc = reserve(ctx, m->d_poses, pose_bytes))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(m->d_poses.p, poses + 16 * first, pose_bytes, hipMemcpyHostToDevice, s));
    return ICPMI_OK;
}

// Queue, for frames [first, last) (first < last): map_queue_tables, and k_map_world into world (rows x 3) and / or keys
// (rows), row 0 being frame first's first row.
int map_queue_world(icpmi_map *m, const double *poses, int64_t first, int64_t last, double *world, unsigned long long *keys,
                    const icpmi_grid_config *grid)
{
    icpmi_ctx *ctx = m->ctx;
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = map_queue_tables(m, poses, first, last))) return rc;
    const int64_t t0 = m->tile0[first], nt = m->tile0[last] - t0;
    GridParams g{0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    if (grid) g = GridParams{0.0, 0.0, grid->resolution, grid->height_min, grid->height_max, grid->max_range};
    const bool mask = keys && grid && m->ground_on; // the band is open; the rows that are not OBSTACLE lose their keys
    if (mask) g.height_min = -std::numeric_limits<double>::max(), g.height_max = std::numeric_limits<double>::max();
    if (nt > 0)
        hipLaunchKernelGGL(k_map_world, dim3((unsigned)nt), dim3(256), 0, s, (const double *)m->d_rows.p,
                           (const MapTile *)m->d_tiles.p + t0, (const double *)m->d_poses.p, (int32_t)first, m->row0[first],
                           world, keys, g);
    HIP_TRY(ctx, hipGetLastError());
    const size_t rows = (size_t)(m->row0[last] - m->row0[first]);
    if (mask && rows > 0) {
        hipLaunchKernelGGL(k_ground_mask, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, keys,
                           (const uint8_t *)m->d_labels.p + m->row0[first], rows);
        HIP_TRY(ctx, hipGetLastError());
    }
    return ICPMI_OK;
}

// What icpmi_map_raycast, icpmi_map_raycast_counts and icpmi_map_live_update decide on the host before any device
// work: R, the used frames' table with their sensor cells, and the plane that holds every used frame's window.
// ray_plan is the four steps below over every used frame; icpmi_map_live_update runs them over its new frames only.
struct RayPlan {
    int R = 0;
    int64_t last = 0, rows = 0;      // the used frames [0, last) and the rows they hold
    std::vector<RayFrame> frames;
    RayPlane pl{0, 0, 0, 0, 0};      // set when rows > 0
};

struct RaySpan {                     // of the sensor cells of the frames that hold rows
    int64_t lo_x = INT64_MAX, lo_y = INT64_MAX, hi_x = INT64_MIN, hi_y = INT64_MIN;
};

int ray_plan_grid(icpmi_ctx *ctx, const icpmi_grid_config *grid, int *R)
{
    if (!grid) return fail(ctx, ICPMI_ERR_NULL, "grid is NULL");
    const double res = grid->resolution;
    if (!(std::isfinite(res) && res > 0.0)) return fail(ctx, ICPMI_ERR_ARG, "grid resolution must be finite and positive");
    const double Rd = std::ceil(grid->max_range / res);
    if (!(Rd <= (double)kRayMaxR))
        return fail(ctx, ICPMI_ERR_ARG, "max_range / resolution must be at most %d cells", kRayMaxR);
    *R = Rd > 0.0 ? (int)Rd : 0;
    return ICPMI_OK;
}

// With ground set: label the frames that are not labelled yet (ground.h), in one launch, and wait for their OBSTACLE
// counts.  The labels are indexed by store row; on any error the labelled frames are those from before.
int map_ground_ready(icpmi_map *m)
{
    icpmi_ctx *ctx = m->ctx;
    const int64_t frames = map_frames(m), first = m->ground_frames, nf = frames - first;
    if (!m->ground_on || nf == 0) return ICPMI_OK;
    Range range("icpmi:map_ground_labels");
    hipStream_t s = ctx->stream;
    int rc;
    const size_t used = (size_t)m->row0[first], need = (size_t)m->row0[frames];
    DevBuf grown; // the new label arena, if it has to grow: the labelled frames' bytes move
    struct Drop {
        DevBuf &b;
        ~Drop() { release(b); }
    } drop{grown};
    if (need > m->d_labels.cap) {
        HIP_TRY(ctx, reserve_raw(grown, std::max(need, 2 * m->d_labels.cap)));
        if (used) HIP_TRY(ctx, hipMemcpyAsync(grown.p, m->d_labels.p, used, hipMemcpyDeviceToDevice, s));
    }
    uint8_t *labels = (uint8_t *)(grown.p ? grown.p : m->d_labels.p);
    const size_t tab = sizeof(GroundFrame) * (size_t)nf;
    if ((rc = reserve(ctx, m->d_ground_tab, tab + sizeof(GroundCounts) * (size_t)nf))) return rc;
    std::vector<GroundFrame> table((size_t)nf);
    for (int64_t i = 0; i < nf; ++i) table[(size_t)i] = GroundFrame{m->row0[first + i], (int32_t)(m->row0[first + i + 1] - m->row0[first + i]), 0};
    std::vector<GroundCounts> counts((size_t)nf);
    GroundCounts *counts_d = (GroundCounts *)((char *)m->d_ground_tab.p + tab);
    HIP_TRY(ctx, hipMemcpyAsync(m->d_ground_tab.p, table.data(), tab, hipMemcpyHostToDevice, s));
    if ((rc = ground_queue(ctx, &m->ground, (const double *)m->d_rows.p, (const GroundFrame *)m->d_ground_tab.p, nf, labels, nullptr,
                           nullptr, counts_d)))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(counts.data(), counts_d, sizeof(GroundCounts) * (size_t)nf, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s)); // the labelling's wait: which frames hold an OBSTACLE row
    HIP_TRY(ctx, hipGetLastError());
    if (grown.p) std::swap(m->d_labels, grown); // (the old arena goes with `drop`)
    for (const GroundCounts &c : counts) m->ground_hits.push_back((int32_t)c.n_obstacle);
    m->ground_frames = frames;
    return ICPMI_OK;
}

// Frames [first, last): their sensor cells (each within range), their table entries behind *frames with row0 counted
// from frame `first`'s first row (k_map_world's keys for those frames), and *span widened by those that hold rows.
int ray_plan_frames(icpmi_map *m, const double *poses, double res, int R, int64_t first, int64_t last, RaySpan *span,
                    std::vector<RayFrame> *frames)
{
    // every carved or occupied cell lies within R + 1 cells of a sensor cell
    const double cell_max = 2147483646.0 - R - 6;
    frames->reserve(frames->size() + (size_t)(last - first));
    for (int64_t i = first; i < last; ++i) {
        const double cx = std::floor(poses[16 * i + 3] / res), cy = std::floor(poses[16 * i + 7] / res);
        if (!(std::fabs(cx) <= cell_max && std::fabs(cy) <= cell_max))
            return fail(m->ctx, ICPMI_ERR_ARG, "frame %lld's sensor cell is out of range", (long long)i);
        // (with ground set a frame holds rows if it holds an OBSTACLE row: the others are cast as empty frames)
        const int64_t rows = m->ground_on && m->ground_hits[(size_t)i] == 0 ? 0 : m->row0[i + 1] - m->row0[i];
        frames->push_back(RayFrame{m->row0[i] - m->row0[first], (int32_t)rows, (int32_t)cx, (int32_t)cy, 0});
        if (rows == 0) continue;
        span->lo_x = std::min<int64_t>(span->lo_x, (int64_t)cx), span->hi_x = std::max<int64_t>(span->hi_x, (int64_t)cx);
        span->lo_y = std::min<int64_t>(span->lo_y, (int64_t)cy), span->hi_y = std::max<int64_t>(span->hi_y, (int64_t)cy);
    }
    return ICPMI_OK;
}

// The plane of a span (of at least one frame): every window, and no more than 2^31 - 1 cells with the raster's margin.
int ray_plan_plane(icpmi_ctx *ctx, const RaySpan &sp, int R, RayPlane *pl)
{
    const int64_t W = sp.hi_x - sp.lo_x + 2 * R + 3, H = sp.hi_y - sp.lo_y + 2 * R + 3;
    if ((W + 10) > (int64_t)INT32_MAX / (H + 10)) // the raster is the tight box widened by 5: never more than this
        return fail(ctx, ICPMI_ERR_ARG, "the used frames span %lld x %lld cells: more than 2^31 - 1", (long long)(W + 10),
                    (long long)(H + 10));
    *pl = RayPlane{(int32_t)(sp.lo_x - R - 1), (int32_t)(sp.lo_y - R - 1), (int32_t)W, (int32_t)H, (int32_t)((W + 31) / 32)};
    return ICPMI_OK;
}

int ray_plan(icpmi_map *m, const double *poses, int64_t n_poses, const icpmi_grid_config *grid, int64_t max_frames, RayPlan *out)
{
    icpmi_ctx *ctx = m->ctx;
    int rc, R = 0;
    if ((rc = ray_plan_grid(ctx, grid, &R))) return rc;
    int64_t last = 0;
    if ((rc = map_check_poses(m, poses, n_poses, &last))) return rc;
    if (last > max_frames)
        return fail(ctx, ICPMI_ERR_ARG, "%lld frames would be used: at most %lld", (long long)last, (long long)max_frames);
    if ((rc = map_ground_ready(m))) return rc;
    std::vector<RayFrame> frames;
    RaySpan span;
    if ((rc = ray_plan_frames(m, poses, grid->resolution, R, 0, last, &span, &frames))) return rc;
    // (a frame that holds rows widens the span; with ground set a store with rows may hold no such frame)
    out->R = R, out->last = last, out->rows = span.lo_x <= span.hi_x ? m->row0[last] : 0;
    if (out->rows > 0 && (rc = ray_plan_plane(ctx, span, R, &out->pl))) return rc;
    out->frames = std::move(frames);
    return ICPMI_OK;
}

} // namespace

extern "C" {

int icpmi_map_create(icpmi_ctx *ctx, icpmi_map **out)
{
    int rc;
    if (!out) return fail(ctx, ICPMI_ERR_NULL, "out is NULL");
    *out = nullptr;
    if ((rc = check_common(ctx))) return rc;
    icpmi_map *m = new icpmi_map;
    m->ctx = ctx;
    *out = m;
    return ICPMI_OK;
}

void icpmi_map_destroy(icpmi_map *m)
{
    if (!m) return;
    (void)hipSetDevice(m->ctx->opt.device);
    (void)hipStreamSynchronize(m->ctx->stream);
    for (DevBuf *b : {&m->d_rows, &m->d_tiles, &m->d_poses, &m->d_world, &m->d_ray_frames, &m->d_ray_planes, &m->d_raster,
                      &m->d_raster_next, &m->d_count_plane, &m->d_count_scratch, &m->d_counts, &m->d_counts_next, &m->live.d_plane,
                      &m->live.d_bounds, &m->live.d_windows, &m->live.d_out, &m->d_labels, &m->d_ground_tab, &m->d_static_labels,
                      &m->d_static_tab})
        release(*b);
    delete m;
}

int icpmi_map_add_frame(icpmi_map *m, const double *xyz, int64_t n)
{
    if (!m) return ICPMI_ERR_NULL;
    int rc;
    if ((rc = check_common(m->ctx))) return rc;
    if (!xyz && n != 0) return fail(m->ctx, ICPMI_ERR_NULL, "null argument");
    return map_append(m, xyz, n, hipMemcpyHostToDevice);
}

int icpmi_map_add_frame_device(icpmi_map *m, const double *d_xyz, int64_t n)
{
    if (!m) return ICPMI_ERR_NULL;
    int rc;
    if ((rc = check_common(m->ctx))) return rc;
    if (!d_xyz && n != 0) return fail(m->ctx, ICPMI_ERR_NULL, "null argument");
    return map_append(m, d_xyz, n, hipMemcpyDeviceToDevice);
}

int icpmi_map_add_stream_frame(icpmi_map *m)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (ctx->stream_prev_n < 0) return fail(ctx, ICPMI_ERR_ARG, "no resident frame: call icpmi_stream_push first");
    return map_append(m, ctx->stream_prev.p, ctx->stream_prev_n, hipMemcpyDeviceToDevice);
}

int icpmi_map_size(const icpmi_map *m, int64_t *frames, int64_t *points)
{
    if (!m) return ICPMI_ERR_NULL;
    if (frames) *frames = map_frames(m);
    if (points) *points = m->row0.back();
    return ICPMI_OK;
}

int icpmi_map_world(icpmi_map *m, const double *poses, int64_t n_poses, int64_t first, double *out_xyz, int64_t cap,
                    int64_t *n_out)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!n_out) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (first < 0) return fail(ctx, ICPMI_ERR_ARG, "first < 0");
    int64_t last = 0;
    if ((rc = map_check_poses(m, poses, n_poses, &last))) return rc;
    first = std::min(first, last);
    const int64_t rows = m->row0[last] - m->row0[first];
    *n_out = rows;
    if (!out_xyz || rows == 0) return ICPMI_OK;
    if (cap < rows) return fail(ctx, ICPMI_ERR_CAPACITY, "output holds %lld rows, needs %lld", (long long)cap, (long long)rows);
    Range range("icpmi:map_world");
    const size_t bytes = sizeof(double) * 3 * (size_t)rows;
    if ((rc = reserve(ctx, m->d_world, bytes))) return rc;
    if ((rc = map_queue_world(m, poses, first, last, (double *)m->d_world.p, nullptr, nullptr))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_xyz, m->d_world.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // the call's one wait
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

int icpmi_map_finish(icpmi_map *m, const double *poses, int64_t n_poses, const icpmi_grid_config *grid, double voxel_size,
                     double *map_out, int64_t map_cap, int64_t *n_map, int64_t *n_cells)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (grid && !(grid->resolution > 0.0)) return fail(ctx, ICPMI_ERR_ARG, "grid resolution must be positive");
    int64_t last = 0;
    if ((rc = map_check_poses(m, poses, n_poses, &last))) return rc;
    const bool want_map = map_out && voxel_size > 0.0;
    if (n_map) *n_map = 0;
    const int64_t n64 = m->row0[last];
    if (grid && n64 > 0 && (rc = map_ground_ready(m))) return rc;
    if (n64 == 0 || (!grid && !want_map)) {
        if (grid) ctx->grid_n = 0; // occupied_cells_.clear() and nothing inserted
        if (n_cells) *n_cells = ctx->grid_n;
        return ICPMI_OK;
    }
    Range range("icpmi:map_finish");
    hipStream_t s = ctx->stream;
    const int n = (int)n64;
    const size_t un = (size_t)n;
    double *world = nullptr;
    if (want_map) {
        if ((rc = reserve(ctx, m->d_world, sizeof(double) * 3 * un))) return rc;
        world = (double *)m->d_world.p;
    }
    // rebuild_occupancy_grid (slam_node.cpp:223-229): the keys of every row -> sorted, unique -> the new set, built in
    // grid_out and swapped in only once the whole call has succeeded
    GridKeySort ks{nullptr, nullptr, nullptr, nullptr, n};
    if (grid) {
        if ((rc = reserve(ctx, ctx->grid_in, sizeof(unsigned long long) * 2 * un))) return rc;
        if ((rc = reserve(ctx, ctx->grid_out, sizeof(unsigned long long) * un))) return rc;
        if ((rc = reserve(ctx, ctx->grid_cnt, sizeof(unsigned) * (un + 16)))) return rc;
        ks = GridKeySort{(unsigned long long *)ctx->grid_in.p, (unsigned long long *)ctx->grid_in.p + un,
                         (unsigned long long *)ctx->grid_out.p, (unsigned *)ctx->grid_cnt.p, n};
        if ((rc = grid_sort_reserve(ctx, ks, 0))) return rc;
    }
    if ((rc = map_queue_world(m, poses, 0, last, world, ks.keys, grid))) return rc;
    if (grid) {
        if ((rc = grid_sort_queue(ctx, ks, 0))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_grid, ks.counts + un + 1, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    }
    int64_t rows = 0;
    if (want_map) {
        // publish_global_map (slam_node.cpp:235-238): voxel_downsample(global_map_points_, voxel) on the world rows, in
        // frame then row order.  The filter waits for its voxel count (and with it the set's size) before it queues the
        // centroids.
        const int64_t cap = std::max<int64_t>(0, std::min<int64_t>(n64, map_cap));
        if ((rc = reserve(ctx, ctx->vox_out, sizeof(double) * 3 * (size_t)std::max<int64_t>(cap, 1)))) return rc;
        if ((rc = voxel_downsample_device(ctx, world, n, voxel_size, (double *)ctx->vox_out.p, cap, &rows, false))) return rc;
        if (rows > 0)
            HIP_TRY(ctx, hipMemcpyAsync(map_out, ctx->vox_out.p, sizeof(double) * 3 * (size_t)rows, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipGetLastError());
    if (grid) {
        std::swap(ctx->grid_set, ctx->grid_out);
        ctx->grid_n = (int64_t)ctx->h_grid[0];
    }
    if (n_map) *n_map = rows;
    if (n_cells) *n_cells = ctx->grid_n;
    return ICPMI_OK;
}

static_assert(kRayMaxR == ICPMI_RAYCAST_MAX_R && kRayLdsMaxR == ICPMI_RAYCAST_LDS_MAX_R, "the header states these limits");

int icpmi_map_raycast(icpmi_map *m, const double *poses, int64_t n_poses, const icpmi_grid_config *grid, icpmi_raster_info *info)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    RayPlan plan;
    if ((rc = ray_plan(m, poses, n_poses, grid, INT64_MAX, &plan))) return rc;
    const int R = plan.R;
    const int64_t last = plan.last, n64 = plan.rows;
    const std::vector<RayFrame> &frames = plan.frames;
    icpmi_raster_info out{0, 0, 0, 0, grid->resolution, 0, 0};
    if (n64 > 0) {
        Range range("icpmi:map_raycast");
        hipStream_t s = ctx->stream;
        const RayPlane pl = plan.pl;
        const size_t words = (size_t)pl.wpr * (size_t)pl.h;
        if ((rc = reserve(ctx, ctx->grid_in, sizeof(unsigned long long) * (size_t)n64))) return rc;
        if ((rc = reserve(ctx, m->d_ray_frames, sizeof(RayFrame) * (size_t)last))) return rc;
        if ((rc = reserve(ctx, m->d_ray_planes, sizeof(unsigned) * 2 * words + sizeof(RayBounds)))) return rc;
        unsigned long long *keys = (unsigned long long *)ctx->grid_in.p;
        unsigned *carved = (unsigned *)m->d_ray_planes.p, *occupied = carved + words;
        RayBounds *bounds_d = (RayBounds *)(occupied + words); // (2 * words * 4 bytes: a multiple of 8)
        const RayFrame *frames_d = (const RayFrame *)m->d_ray_frames.p;
        static const RayBounds kNone{INT32_MAX, INT32_MAX, -1, -1, 0, 0};
        HIP_TRY(ctx, hipMemsetAsync(carved, 0, sizeof(unsigned) * 2 * words, s));
        HIP_TRY(ctx, hipMemcpyAsync(bounds_d, &kNone, sizeof(RayBounds), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(m->d_ray_frames.p, frames.data(), sizeof(RayFrame) * (size_t)last, hipMemcpyHostToDevice, s));
        if ((rc = map_queue_world(m, poses, 0, last, nullptr, keys, grid))) return rc;
        if (R <= kRayLdsMaxR) {
            const size_t window = sizeof(unsigned) * (size_t)ray_window_words(R);
            if (window > 64 * 1024) // (R > 351) dynamic LDS past 64 KiB has to be allowed first
                HIP_TRY(ctx, hipFuncSetAttribute((const void *)k_ray_carve_lds, hipFuncAttributeMaxDynamicSharedMemorySize, kRayLdsBytes));
            hipLaunchKernelGGL(k_ray_carve_lds, dim3((unsigned)last), dim3(kRayThreads), window, s,
                               (const unsigned long long *)keys, frames_d, R, pl, carved, occupied);
        } else
            hipLaunchKernelGGL(k_ray_carve_global, dim3((unsigned)m->tile0[last]), dim3(256), 0, s, (const unsigned long long *)keys,
                               (const MapTile *)m->d_tiles.p, frames_d, R, pl, carved, occupied);
        HIP_TRY(ctx, hipGetLastError());
        const unsigned blocks = (unsigned)std::min<size_t>((words + 255) / 256, 1024);
        hipLaunchKernelGGL(k_ray_bounds, dim3(blocks), dim3(256), 0, s, (const unsigned *)carved, (const unsigned *)occupied, pl,
                           bounds_d);
        HIP_TRY(ctx, hipGetLastError());
        RayBounds b{};
        HIP_TRY(ctx, hipMemcpyAsync(&b, bounds_d, sizeof(RayBounds), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s)); // the first wait: the raster's size
        if (b.max_x >= 0) {
            out.min_x = pl.x0 + b.min_x - 5;
            out.min_y = pl.y0 + b.min_y - 5;
            out.width = b.max_x - b.min_x + 11;
            out.height = b.max_y - b.min_y + 11;
            out.n_occupied = (int64_t)b.n_occupied;
            out.n_free = (int64_t)b.n_free;
            const size_t cells = (size_t)out.width * (size_t)out.height;
            if ((rc = reserve(ctx, m->d_raster_next, cells))) return rc;
            hipLaunchKernelGGL(k_ray_raster, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, (const unsigned *)carved,
                               (const unsigned *)occupied, pl, b.min_x - 5, b.min_y - 5, out.width, out.height,
                               (int8_t *)m->d_raster_next.p);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(s)); // the second: the raster is complete before it replaces the last one
            std::swap(m->d_raster, m->d_raster_next);
        }
    }
    m->raster = out;
    if (info) *info = out;
    return ICPMI_OK;
}

int icpmi_map_raster(icpmi_map *m, int8_t *data, int64_t cap, icpmi_raster_info *info)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (info) *info = m->raster;
    if (!data) return ICPMI_OK;
    const int64_t cells = (int64_t)m->raster.width * (int64_t)m->raster.height;
    if (cap < cells) return fail(ctx, ICPMI_ERR_CAPACITY, "data holds %lld cells, needs %lld", (long long)cap, (long long)cells);
    if (cells == 0) return ICPMI_OK;
    HIP_TRY(ctx, hipMemcpyAsync(data, m->d_raster.p, (size_t)cells, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // the call's one wait
    return ICPMI_OK;
}

static_assert(kCountMaxFrames == ICPMI_RAYCOUNT_MAX_FRAMES && kCountLdsMaxR == ICPMI_RAYCOUNT_LDS_MAX_R, "the header states these limits");

// hits (uint16), misses (uint16), probability (int8) of `cells` cells, in that order in one buffer
static size_t counts_bytes(size_t cells) { return 5 * cells; }

int icpmi_map_raycast_counts(icpmi_map *m, const double *poses, int64_t n_poses, const icpmi_grid_config *grid,
                             icpmi_counts_info *info)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    RayPlan plan;
    if ((rc = ray_plan(m, poses, n_poses, grid, kCountMaxFrames, &plan))) return rc;
    const int R = plan.R;
    const int64_t last = plan.last, n64 = plan.rows;
    icpmi_counts_info out{0, 0, 0, 0, grid->resolution, 0, 0, 0, 0, (int32_t)last, 0};
    if (n64 > 0) {
        Range range("icpmi:map_raycast_counts");
        hipStream_t s = ctx->stream;
        const RayPlane pl = plan.pl;
        const size_t plane_cells = (size_t)pl.w * (size_t)pl.h;
        const size_t pair = sizeof(unsigned) * 2 * (size_t)ray_window_words(R);
        const bool lds = R <= kCountLdsMaxR;
        const int groups = lds ? (int)last : count_scratch_groups(R, last);
        if ((rc = reserve(ctx, ctx->grid_in, sizeof(unsigned long long) * (size_t)n64))) return rc;
        if ((rc = reserve(ctx, m->d_ray_frames, sizeof(RayFrame) * (size_t)last))) return rc;
        if ((rc = reserve(ctx, m->d_count_plane, sizeof(unsigned) * plane_cells + 8 + sizeof(CountBounds)))) return rc;
        if (!lds && (rc = reserve(ctx, m->d_count_scratch, pair * (size_t)groups))) return rc;
        unsigned long long *keys = (unsigned long long *)ctx->grid_in.p;
        unsigned *plane = (unsigned *)m->d_count_plane.p;
        CountBounds *bounds_d = (CountBounds *)((char *)plane + (sizeof(unsigned) * plane_cells + 7) / 8 * 8);
        const RayFrame *frames_d = (const RayFrame *)m->d_ray_frames.p;
        static const CountBounds kNone{INT32_MAX, INT32_MAX, -1, -1, 0, 0, 0, 0};
        HIP_TRY(ctx, hipMemsetAsync(plane, 0, sizeof(unsigned) * plane_cells, s));
        HIP_TRY(ctx, hipMemcpyAsync(bounds_d, &kNone, sizeof(CountBounds), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(m->d_ray_frames.p, plan.frames.data(), sizeof(RayFrame) * (size_t)last, hipMemcpyHostToDevice, s));
        if ((rc = map_queue_world(m, poses, 0, last, nullptr, keys, grid))) return rc;
        if (lds) {
            if (R > kCountLdsPlainMaxR) // dynamic LDS past 64 KiB has to be allowed first
                HIP_TRY(ctx, hipFuncSetAttribute((const void *)k_ray_count<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kRayLdsBytes));
            hipLaunchKernelGGL(k_ray_count<true>, dim3((unsigned)groups), dim3(kRayThreads), pair, s, (const unsigned long long *)keys,
                               frames_d, (int)last, R, pl, (unsigned *)nullptr, plane);
        } else {
            HIP_TRY(ctx, hipMemsetAsync(m->d_count_scratch.p, 0, pair * (size_t)groups, s));
            hipLaunchKernelGGL(k_ray_count<false>, dim3((unsigned)groups), dim3(kRayThreads), 0, s, (const unsigned long long *)keys,
                               frames_d, (int)last, R, pl, (unsigned *)m->d_count_scratch.p, plane);
        }
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_count_bounds, dim3((unsigned)std::min<int32_t>(pl.h, 1024)), dim3(256), 0, s, (const unsigned *)plane, pl,
                           bounds_d);
        HIP_TRY(ctx, hipGetLastError());
        CountBounds b{};
        HIP_TRY(ctx, hipMemcpyAsync(&b, bounds_d, sizeof(CountBounds), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s)); // the first wait: the arrays' size
        if (b.max_x >= 0) {
            out.min_x = pl.x0 + b.min_x - 5;
            out.min_y = pl.y0 + b.min_y - 5;
            out.width = b.max_x - b.min_x + 11;
            out.height = b.max_y - b.min_y + 11;
            out.n_observed = (int64_t)b.n_observed;
            out.n_hit_cells = (int64_t)b.n_hit_cells;
            out.max_hits = b.max_hits;
            out.max_misses = b.max_misses;
            const size_t cells = (size_t)out.width * (size_t)out.height;
            if ((rc = reserve(ctx, m->d_counts_next, counts_bytes(cells)))) return rc;
            uint16_t *hits = (uint16_t *)m->d_counts_next.p;
            hipLaunchKernelGGL(k_count_raster, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, (const unsigned *)plane, pl,
                               b.min_x - 5, b.min_y - 5, out.width, out.height, hits, hits + cells, (int8_t *)(hits + 2 * cells));
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(s)); // the second: the arrays are complete before they replace the last ones
            std::swap(m->d_counts, m->d_counts_next);
        }
    }
    m->counts = out;
    if (info) *info = out;
    return ICPMI_OK;
}

int icpmi_map_counts(icpmi_map *m, uint16_t *hits, uint16_t *misses, int8_t *probability, int64_t cap, icpmi_counts_info *info)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (info) *info = m->counts;
    if (!hits && !misses && !probability) return ICPMI_OK;
    const int64_t cells = (int64_t)m->counts.width * (int64_t)m->counts.height;
    if (cap < cells) return fail(ctx, ICPMI_ERR_CAPACITY, "the arrays hold %lld cells, need %lld", (long long)cap, (long long)cells);
    if (cells == 0) return ICPMI_OK;
    const char *src = (const char *)m->d_counts.p;
    const size_t n = (size_t)cells;
    if (hits) HIP_TRY(ctx, hipMemcpyAsync(hits, src, 2 * n, hipMemcpyDeviceToHost, ctx->stream));
    if (misses) HIP_TRY(ctx, hipMemcpyAsync(misses, src + 2 * n, 2 * n, hipMemcpyDeviceToHost, ctx->stream));
    if (probability) HIP_TRY(ctx, hipMemcpyAsync(probability, src + 4 * n, n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // the call's one wait
    return ICPMI_OK;
}

} // extern "C"

// ---- the counts kept while the node drives (live_counts.h, live_plane.h) ----

namespace {

const CountBounds kCountNone{INT32_MAX, INT32_MAX, -1, -1, 0, 0, 0, 0};

RayPlane live_ray_plane(const LiveBox &b)
{
    return RayPlane{(int32_t)b.x0, (int32_t)b.y0, (int32_t)b.w, (int32_t)b.h, (int32_t)((b.w + 31) / 32)};
}

// What an update reports: icpmi_map_raycast_counts' info from the running bounds, and the plane's box.
void live_fill_info(const LiveCounts &L, int64_t used, icpmi_live_info *out)
{
    icpmi_counts_info c{0, 0, 0, 0, L.grid.resolution, 0, 0, 0, 0, (int32_t)used, 0};
    const CountBounds &b = L.bounds;
    if (L.box.w > 0 && b.max_x >= 0) {
        c.min_x = (int32_t)L.box.x0 + b.min_x - 5;
        c.min_y = (int32_t)L.box.y0 + b.min_y - 5;
        c.width = b.max_x - b.min_x + 11;
        c.height = b.max_y - b.min_y + 11;
        c.n_observed = (int64_t)b.n_observed;
        c.n_hit_cells = (int64_t)b.n_hit_cells;
        c.max_hits = b.max_hits;
        c.max_misses = b.max_misses;
    }
    out->counts = c;
    out->plane_x0 = (int32_t)L.box.x0, out->plane_y0 = (int32_t)L.box.y0;
    out->plane_w = (int32_t)L.box.w, out->plane_h = (int32_t)L.box.h;
}

// An update's device work and its one wait: frames [first, used) (`frames`: their table, rows counted from frame
// first's; they hold rows) are cast into the plane, which becomes `box`.  rebuild: the plane is zeroed first.  `old`
// takes the buffers to release after the wait; *b the bounds after it.
int live_cast(icpmi_map *m, const double *poses, const icpmi_grid_config *grid, int R, bool rebuild, int64_t first, int64_t used,
              const std::vector<RayFrame> &frames, const LiveBox &box, bool *moved, std::vector<DevBuf> &old, CountBounds *b)
{
    icpmi_ctx *ctx = m->ctx;
    LiveCounts &L = m->live;
    hipStream_t s = ctx->stream;
    int rc;
    Range range("icpmi:map_live_update");
    const int64_t rows = m->row0[used] - m->row0[first];
    const size_t plane_bytes = sizeof(unsigned) * (size_t)box.w * (size_t)box.h;
    if ((rc = reserve(ctx, ctx->grid_in, sizeof(unsigned long long) * (size_t)rows))) return rc;
    if ((rc = reserve(ctx, L.d_bounds, sizeof(CountBounds)))) return rc;
    CountBounds *bounds_d = (CountBounds *)L.d_bounds.p;
    if (rebuild || L.box.w == 0) {  // a fresh plane
        if ((rc = reserve(ctx, L.d_plane, plane_bytes))) return rc;
        HIP_TRY(ctx, hipMemsetAsync(L.d_plane.p, 0, plane_bytes, s));
        HIP_TRY(ctx, hipMemcpyAsync(bounds_d, &kCountNone, sizeof(CountBounds), hipMemcpyHostToDevice, s));
    } else if (box.x0 != L.box.x0 || box.y0 != L.box.y0 || box.w != L.box.w || box.h != L.box.h) {
        DevBuf grown;               // the plane grows: its words move into a larger zeroed one
        HIP_TRY(ctx, reserve_raw(grown, plane_bytes));
        old.push_back(L.d_plane);
        L.d_plane = grown;
        HIP_TRY(ctx, hipMemsetAsync(grown.p, 0, plane_bytes, s));
        hipLaunchKernelGGL(k_plane_move, dim3((unsigned)std::min<int64_t>(L.box.h, 2048)), dim3(256), 0, s,
                           (const unsigned *)old.back().p, (int)L.box.w, (int)L.box.h, (unsigned *)grown.p, (int)box.w,
                           (int)(L.box.x0 - box.x0), (int)(L.box.y0 - box.y0), bounds_d);
        HIP_TRY(ctx, hipGetLastError());
        *moved = true;
    }
    L.box = box;
    const RayPlane pl = live_ray_plane(box);
    unsigned *plane = (unsigned *)L.d_plane.p;
    unsigned long long *keys = (unsigned long long *)ctx->grid_in.p;
    if ((rc = map_queue_world(m, poses, first, used, nullptr, keys, grid))) return rc;
    const int64_t nf = used - first;
    int64_t held = 0;
    for (const RayFrame &f : frames) held += f.rows > 0;
    const size_t pair = sizeof(unsigned) * 2 * (size_t)ray_window_words(R);
    const bool lds = R <= kCountLdsMaxR;
    if (rebuild || !lds || held > kLiveBatchFrames) {
        // icpmi_map_raycast_counts' kernels, aimed at the live plane: their adds are atomic, so they may fall on counts
        // already there; the bounds are then counted again over the whole plane
        const int groups = lds ? (int)nf : count_scratch_groups(R, nf);
        if ((rc = reserve(ctx, m->d_ray_frames, sizeof(RayFrame) * (size_t)nf))) return rc;
        if (!lds && (rc = reserve(ctx, m->d_count_scratch, pair * (size_t)groups))) return rc;
        const RayFrame *frames_d = (const RayFrame *)m->d_ray_frames.p;
        HIP_TRY(ctx, hipMemcpyAsync(m->d_ray_frames.p, frames.data(), sizeof(RayFrame) * (size_t)nf, hipMemcpyHostToDevice, s));
        if (lds) {
            if (R > kCountLdsPlainMaxR)
                HIP_TRY(ctx, hipFuncSetAttribute((const void *)k_ray_count<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kRayLdsBytes));
            hipLaunchKernelGGL(k_ray_count<true>, dim3((unsigned)groups), dim3(kRayThreads), pair, s, (const unsigned long long *)keys,
                               frames_d, (int)nf, R, pl, (unsigned *)nullptr, plane);
        } else {
            HIP_TRY(ctx, hipMemsetAsync(m->d_count_scratch.p, 0, pair * (size_t)groups, s));
            hipLaunchKernelGGL(k_ray_count<false>, dim3((unsigned)groups), dim3(kRayThreads), 0, s, (const unsigned long long *)keys,
                               frames_d, (int)nf, R, pl, (unsigned *)m->d_count_scratch.p, plane);
        }
        HIP_TRY(ctx, hipGetLastError());
        if (!rebuild) HIP_TRY(ctx, hipMemcpyAsync(bounds_d, &kCountNone, sizeof(CountBounds), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_count_bounds, dim3((unsigned)std::min<int32_t>(pl.h, 1024)), dim3(256), 0, s, (const unsigned *)plane, pl,
                           bounds_d);
        HIP_TRY(ctx, hipGetLastError());
    } else {
        if (pair > L.d_windows.cap) L.windows_clean = false;
        if ((rc = reserve(ctx, L.d_windows, pair))) return rc;
        if (!L.windows_clean) HIP_TRY(ctx, hipMemsetAsync(L.d_windows.p, 0, L.d_windows.cap, s));
        L.windows_clean = false;    // until the call's wait has shown that every k_live_apply ran
        if (R > kCountLdsPlainMaxR) // dynamic LDS past 64 KiB has to be allowed first
            HIP_TRY(ctx, hipFuncSetAttribute((const void *)k_live_carve, hipFuncAttributeMaxDynamicSharedMemorySize, kRayLdsBytes));
        unsigned *win = (unsigned *)L.d_windows.p;
        const int tasks = (ray_window_words(R) + 1) / 2, per = kLiveApplyThreads / 64;
        const unsigned apply_groups = (unsigned)std::min(kLiveApplyGroups, (tasks + per - 1) / per);
        for (const RayFrame &f : frames) {
            if (f.rows == 0) continue;
            const int wx0 = (int)((int64_t)f.sx - (R + 1) - box.x0), wy0 = (int)((int64_t)f.sy - (R + 1) - box.y0);
            hipLaunchKernelGGL(k_live_carve, dim3((unsigned)live_carve_groups(f.rows)), dim3(kRayThreads), pair, s,
                               (const unsigned long long *)keys, f, R, wx0 & 31, live_carve_share(f.rows), win);
            hipLaunchKernelGGL(k_live_apply, dim3(apply_groups), dim3(kLiveApplyThreads), 0, s, win, R, wx0, wy0, pl, plane, bounds_d);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipMemcpyAsync(b, bounds_d, sizeof(CountBounds), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s)); // the call's one wait
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

} // namespace

extern "C" {

int icpmi_map_live_update(icpmi_map *m, const double *poses, int64_t n_poses, const icpmi_grid_config *grid, icpmi_live_info *info)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    LiveCounts &L = m->live;
    int rc, R = 0;
    if ((rc = check_common(ctx))) return rc;
    // ray_plan's steps, over the frames this call would cast
    if ((rc = ray_plan_grid(ctx, grid, &R))) return rc;
    int64_t used = 0;
    if ((rc = map_check_count(m, poses, n_poses, &used))) return rc;
    const bool inc = L.valid && memcmp(&L.grid, grid, sizeof(*grid)) == 0 && used >= L.n_cast &&
                     (L.n_cast == 0 || memcmp(poses, L.poses.data(), sizeof(double) * 16 * (size_t)L.n_cast) == 0);
    const int64_t first = inc ? L.n_cast : 0;
    if ((rc = map_check_finite(m, poses, first, used))) return rc;
    if (used > kCountMaxFrames)
        return fail(ctx, ICPMI_ERR_ARG, "%lld frames would be used: at most %lld", (long long)used, (long long)kCountMaxFrames);
    if ((rc = map_ground_ready(m))) return rc;
    RaySpan span;
    if (inc) span = RaySpan{L.span[0], L.span[1], L.span[2], L.span[3]};
    std::vector<RayFrame> frames;
    if ((rc = ray_plan_frames(m, poses, grid->resolution, R, first, used, &span, &frames))) return rc;
    RayPlane exact{0, 0, 0, 0, 0};
    // (a frame that holds rows has widened the span: without ground, row0[used] > 0 says the same)
    if (span.lo_x <= span.hi_x && (rc = ray_plan_plane(ctx, span, R, &exact))) return rc;
    bool new_rows = false;              // does a frame to cast hold rows?
    for (const RayFrame &f : frames) new_rows |= f.rows > 0;
    icpmi_live_info out{};
    if (inc && used == L.n_cast) {  // nothing new
        out = L.info;
        out.frames_cast = 0, out.rebuilt = 0, out.moved = 0;
        L.info = out;
        if (info) *info = out;
        return ICPMI_OK;
    }
    LiveBox box = inc ? L.box : LiveBox{exact.x0, exact.y0, exact.w, exact.h};
    if (inc)
        for (const RayFrame &f : frames)
            if (f.rows > 0) box = live_plane_grow(box, live_window(f.sx, f.sy, R));
    if (box.w > INT32_MAX || box.h > INT32_MAX) return fail(ctx, ICPMI_ERR_ARG, "the live plane would be too wide");
    out.frames_cast = used - first;
    out.rebuilt = !inc && L.n_cast > 0;
    // from here on the remembered state stands only once the call has succeeded
    L.valid = false;
    L.info = icpmi_live_info{};
    CountBounds b = L.bounds;
    bool moved = false;
    if (new_rows) {
        std::vector<DevBuf> old;
        rc = live_cast(m, poses, grid, R, !inc, first, used, frames, box, &moved, old, &b);
        for (DevBuf &o : old) release(o);
        if (rc) return rc;
        L.windows_clean = true;
    } else if (!inc) {              // no used frame holds a row: no plane
        L.box = LiveBox{};
        b = kCountNone;
    }
    L.grid = *grid, L.R = R;
    if (!inc) L.poses.clear();
    L.poses.insert(L.poses.end(), poses + 16 * first, poses + 16 * used);
    L.n_cast = used;
    L.span[0] = span.lo_x, L.span[1] = span.lo_y, L.span[2] = span.hi_x, L.span[3] = span.hi_y;
    L.bounds = b;
    L.valid = true;
    out.moved = moved;
    live_fill_info(L, used, &out);
    L.info = out;
    if (info) *info = out;
    return ICPMI_OK;
}

int icpmi_map_live_counts(icpmi_map *m, uint16_t *hits, uint16_t *misses, int8_t *probability, int64_t cap, icpmi_live_info *info)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    LiveCounts &L = m->live;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (info) *info = L.info;
    if (!hits && !misses && !probability) return ICPMI_OK;
    const icpmi_counts_info &c = L.info.counts;
    const int64_t cells = (int64_t)c.width * (int64_t)c.height;
    if (cap < cells) return fail(ctx, ICPMI_ERR_CAPACITY, "the arrays hold %lld cells, need %lld", (long long)cap, (long long)cells);
    if (cells == 0) return ICPMI_OK;
    Range range("icpmi:map_live_counts");
    hipStream_t s = ctx->stream;
    const size_t n = (size_t)cells;
    if ((rc = reserve(ctx, L.d_out, counts_bytes(n)))) return rc;
    uint16_t *out = (uint16_t *)L.d_out.p;
    hipLaunchKernelGGL(k_count_raster, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const unsigned *)L.d_plane.p,
                       live_ray_plane(L.box), L.bounds.min_x - 5, L.bounds.min_y - 5, c.width, c.height, out, out + n,
                       (int8_t *)(out + 2 * n));
    HIP_TRY(ctx, hipGetLastError());
    const char *src = (const char *)L.d_out.p;
    if (hits) HIP_TRY(ctx, hipMemcpyAsync(hits, src, 2 * n, hipMemcpyDeviceToHost, s));
    if (misses) HIP_TRY(ctx, hipMemcpyAsync(misses, src + 2 * n, 2 * n, hipMemcpyDeviceToHost, s));
    if (probability) HIP_TRY(ctx, hipMemcpyAsync(probability, src + 4 * n, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s)); // the call's one wait
    return ICPMI_OK;
}

int icpmi_map_live_clear(icpmi_map *m)
{
    if (!m) return ICPMI_ERR_NULL;
    LiveCounts &L = m->live;
    L.valid = false;
    L.n_cast = 0;
    L.poses.clear();
    L.box = LiveBox{};
    L.bounds = kCountNone;
    L.info = icpmi_live_info{};
    return ICPMI_OK;            // the buffers stay for the next plane
}

int icpmi_map_set_ground(icpmi_map *m, const icpmi_ground_config *cfg)
{
    if (!m) return ICPMI_ERR_NULL;
    int rc;
    if (cfg && (rc = ground_check(m->ctx, cfg))) return rc;
    m->ground_on = cfg != nullptr;
    if (cfg) m->ground = *cfg;
    m->ground_frames = 0;       // the labels are formed again by the next call that needs them
    m->ground_hits.clear();
    m->live.valid = false;      // the next icpmi_map_live_update rebuilds
    return ICPMI_OK;
}

int icpmi_map_ground_labels(icpmi_map *m, int64_t frame, uint8_t *labels, int64_t cap, int64_t *n_out)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!n_out) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (!m->ground_on) return fail(ctx, ICPMI_ERR_ARG, "no ground config is set: call icpmi_map_set_ground first");
    if (frame < 0 || frame >= map_frames(m)) return fail(ctx, ICPMI_ERR_ARG, "frame %lld is out of range", (long long)frame);
    const int64_t rows = m->row0[frame + 1] - m->row0[frame];
    *n_out = rows;
    if (!labels) return ICPMI_OK;
    if (cap < rows) return fail(ctx, ICPMI_ERR_CAPACITY, "labels holds %lld rows, needs %lld", (long long)cap, (long long)rows);
    if ((rc = map_ground_ready(m))) return rc;
    if (rows == 0) return ICPMI_OK;
    HIP_TRY(ctx, hipMemcpyAsync(labels, (const uint8_t *)m->d_labels.p + m->row0[frame], (size_t)rows, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ICPMI_OK;
}

} // extern "C"

// ---- the static map: the point products without the rows the counts outvote (static_map.h) ----

namespace {

static_assert(sizeof(icpmi_static_rule) == 16 && sizeof(icpmi_static_info) == 32 + sizeof(icpmi_live_info), "the header's layout");

struct StaticRun {
    int64_t t_first = 0, t_end = 0; // the tiles of frames [first, used)
    unsigned base = 0;              // the kept rows before frame first
    int64_t n = 0;                  // the kept rows of frames [first, used)
    icpmi_static_info info{};
};

int static_check_rule(icpmi_ctx *ctx, const icpmi_static_rule *rule)
{
    if (!rule) return fail(ctx, ICPMI_ERR_NULL, "rule is NULL");
    if (rule->min_probability < 0 || rule->min_probability > 100)
        return fail(ctx, ICPMI_ERR_ARG, "rule: min_probability must lie in [0, 100]");
    if (rule->min_observations < 1) return fail(ctx, ICPMI_ERR_ARG, "rule: min_observations must be at least 1");
    if (rule->reserved != 0) return fail(ctx, ICPMI_ERR_ARG, "rule: reserved must be 0");
    return ICPMI_OK;
}

// The live counts brought up to date (icpmi_map_live_update itself), then the labels of every used row against the
// live plane, the tiles' kept rows and their exclusive sums, and one wait for the totals.  d_poses then holds the used
// frames' poses from frame 0 on, for static_queue_world.
int static_labels_run(icpmi_map *m, const double *poses, int64_t n_poses, const icpmi_grid_config *grid, const icpmi_static_rule *rule,
                      int64_t first, StaticRun *run)
{
    icpmi_ctx *ctx = m->ctx;
    hipStream_t s = ctx->stream;
    int rc;
    icpmi_live_info live{};
    if ((rc = icpmi_map_live_update(m, poses, n_poses, grid, &live))) return rc;
    const LiveCounts &L = m->live;
    const int64_t used = L.n_cast, rows = m->row0[used];
    first = std::min(first, used);
    run->t_first = m->tile0[first], run->t_end = m->tile0[used];
    run->info = icpmi_static_info{rows, 0, 0, rows, live};
    m->static_frames = -1;          // until this call's labels stand
    if (rows == 0) {
        m->static_frames = used;
        return ICPMI_OK;
    }
    Range range("icpmi:map_static_labels");
    const size_t T = (size_t)run->t_end;
    // kept (T + 1 words, the last one 0) | their exclusive sums (T + 1 words: the last one is the total) | StaticTotals
    const size_t words = 2 * (T + 1);
    if ((rc = reserve(ctx, m->d_static_labels, (size_t)rows))) return rc;
    if ((rc = reserve(ctx, m->d_static_tab, sizeof(unsigned) * words + sizeof(StaticTotals)))) return rc;
    unsigned *kept = (unsigned *)m->d_static_tab.p, *offs = kept + (T + 1);
    StaticTotals *totals_d = (StaticTotals *)(kept + words);
    size_t scan_bytes = 0;
    HIP_TRY(ctx, exclusive_sum_u32(nullptr, &scan_bytes, kept, offs, (unsigned)(T + 1), s));
    if ((rc = reserve(ctx, ctx->sort_tmp, scan_bytes))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(kept + T, 0, sizeof(unsigned), s));
    HIP_TRY(ctx, hipMemsetAsync(totals_d, 0, sizeof(StaticTotals), s));
    if ((rc = map_queue_tables(m, poses, 0, used))) return rc;
    GridParams g{0.0, 0.0, grid->resolution, grid->height_min, grid->height_max, grid->max_range};
    if (m->ground_on) // as map_queue_world: the band is open, the rows that are not OBSTACLE mark nothing
        g.height_min = -std::numeric_limits<double>::max(), g.height_max = std::numeric_limits<double>::max();
    const StaticPlane pl{L.box.w > 0 ? (const unsigned *)L.d_plane.p : nullptr, (long long)L.box.x0, (long long)L.box.y0,
                         (long long)L.box.w, (long long)L.box.h};
    hipLaunchKernelGGL(k_static_label, dim3((unsigned)T), dim3(256), 0, s, (const double *)m->d_rows.p, (const MapTile *)m->d_tiles.p,
                       (const double *)m->d_poses.p, m->ground_on ? (const uint8_t *)m->d_labels.p : (const uint8_t *)nullptr, pl, g,
                       StaticRuleK{rule->min_probability, rule->min_observations}, (uint8_t *)m->d_static_labels.p, kept, totals_d);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, exclusive_sum_u32(ctx->sort_tmp.p, &scan_bytes, kept, offs, (unsigned)(T + 1), s));
    unsigned ends[2] = {0, 0};
    StaticTotals totals{0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(&ends[0], offs + run->t_first, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(&ends[1], offs + T, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(&totals, totals_d, sizeof(StaticTotals), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s)); // the labels' wait: how many rows are kept
    HIP_TRY(ctx, hipGetLastError());
    if ((int64_t)ends[1] != rows - (int64_t)totals.dropped || ends[0] > ends[1])
        return fail(ctx, ICPMI_ERR_HIP, "static map: the tiles' kept rows (%u) and the dropped rows (%llu) do not add up to %lld",
                    ends[1], totals.dropped, (long long)rows);
    m->static_frames = used;
    run->base = ends[0], run->n = (int64_t)(ends[1] - ends[0]);
    run->info.voting = (int64_t)totals.voting, run->info.dropped = (int64_t)totals.dropped;
    run->info.kept = rows - run->info.dropped;
    return ICPMI_OK;
}

// Queue k_static_world for the tiles of frames [first, used) into world (run.n rows, run.n > 0), behind static_labels_run.
int static_queue_world(icpmi_map *m, const StaticRun &run, double *world)
{
    icpmi_ctx *ctx = m->ctx;
    const size_t T = (size_t)run.t_end;
    const unsigned *offs = (const unsigned *)m->d_static_tab.p + (T + 1);
    hipLaunchKernelGGL(k_static_world, dim3((unsigned)(run.t_end - run.t_first)), dim3(256), 0, ctx->stream, (const double *)m->d_rows.p,
                       (const MapTile *)m->d_tiles.p + run.t_first, (const double *)m->d_poses.p,
                       (const uint8_t *)m->d_static_labels.p, offs + run.t_first, run.base, world);
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

} // namespace

extern "C" {

int icpmi_map_world_static(icpmi_map *m, const double *poses, int64_t n_poses, const icpmi_grid_config *grid,
                           const icpmi_static_rule *rule, int64_t first, double *out_xyz, int64_t cap, int64_t *n_out,
                           icpmi_static_info *info)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if ((rc = static_check_rule(ctx, rule))) return rc;
    if (!n_out) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (first < 0) return fail(ctx, ICPMI_ERR_ARG, "first < 0");
    StaticRun run;
    if ((rc = static_labels_run(m, poses, n_poses, grid, rule, first, &run))) return rc;
    *n_out = run.n;
    if (info) *info = run.info;
    if (!out_xyz || run.n == 0) return ICPMI_OK;
    if (cap < run.n) return fail(ctx, ICPMI_ERR_CAPACITY, "output holds %lld rows, needs %lld", (long long)cap, (long long)run.n);
    Range range("icpmi:map_world_static");
    const size_t bytes = sizeof(double) * 3 * (size_t)run.n;
    if ((rc = reserve(ctx, m->d_world, bytes))) return rc;
    if ((rc = static_queue_world(m, run, (double *)m->d_world.p))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_xyz, m->d_world.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // the points' wait
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

int icpmi_map_finish_static(icpmi_map *m, const double *poses, int64_t n_poses, const icpmi_grid_config *grid,
                            const icpmi_static_rule *rule, double voxel_size, double *map_out, int64_t map_cap, int64_t *n_map,
                            icpmi_static_info *info)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if ((rc = static_check_rule(ctx, rule))) return rc;
    StaticRun run;
    if ((rc = static_labels_run(m, poses, n_poses, grid, rule, 0, &run))) return rc;
    if (n_map) *n_map = 0;
    if (info) *info = run.info;
    if (!(map_out && voxel_size > 0.0) || run.n == 0) return ICPMI_OK;
    Range range("icpmi:map_finish_static");
    hipStream_t s = ctx->stream;
    if ((rc = reserve(ctx, m->d_world, sizeof(double) * 3 * (size_t)run.n))) return rc;
    if ((rc = static_queue_world(m, run, (double *)m->d_world.p))) return rc;
    // publish_global_map (slam_node.cpp:235-238) over the kept rows, in frame then row order: icpmi_map_finish's tail
    int64_t rows = 0;
    const int64_t cap = std::max<int64_t>(0, std::min<int64_t>(run.n, map_cap));
    if ((rc = reserve(ctx, ctx->vox_out, sizeof(double) * 3 * (size_t)std::max<int64_t>(cap, 1)))) return rc;
    if ((rc = voxel_downsample_device(ctx, (const double *)m->d_world.p, (int)run.n, voxel_size, (double *)ctx->vox_out.p, cap, &rows, false)))
        return rc;
    if (rows > 0) HIP_TRY(ctx, hipMemcpyAsync(map_out, ctx->vox_out.p, sizeof(double) * 3 * (size_t)rows, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipGetLastError());
    if (n_map) *n_map = rows;
    return ICPMI_OK;
}

int icpmi_map_static_labels(icpmi_map *m, int64_t frame, uint8_t *labels, int64_t cap, int64_t *n_out)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!n_out) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (m->static_frames < 0) return fail(ctx, ICPMI_ERR_ARG, "no labels yet: call icpmi_map_world_static or icpmi_map_finish_static first");
    if (frame < 0 || frame >= m->static_frames)
        return fail(ctx, ICPMI_ERR_ARG, "frame %lld was not used by the call that formed the labels (%lld frames)", (long long)frame,
                    (long long)m->static_frames);
    const int64_t rows = m->row0[frame + 1] - m->row0[frame];
    *n_out = rows;
    if (!labels) return ICPMI_OK;
    if (cap < rows) return fail(ctx, ICPMI_ERR_CAPACITY, "labels holds %lld rows, needs %lld", (long long)cap, (long long)rows);
    if (rows == 0) return ICPMI_OK;
    HIP_TRY(ctx, hipMemcpyAsync(labels, (const uint8_t *)m->d_static_labels.p + m->row0[frame], (size_t)rows, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ICPMI_OK;
}

} // extern "C"

// ======================================================================================================================
// Loop-closure detection over the store (core/loop_closure.hpp:41-148; loop_store.h): the entries' descriptors and
// labels in device memory, the rows in the map's arena.  Per detect: one upload of the pending entries' (row0, rows,
// label), k_loop_describe for them, k_loop_candidates, one wait; then the candidates' verifications.  With the yaw
// guess on (icpmi_loop_set_yaw_guess) the candidate pass is k_loop_candidates_shift and each verification starts from
// its candidate's icpmi_sc_shift_transform.

struct icpmi_loop {
    icpmi_map *map = nullptr;
    icpmi_loop_config cfg{};
    DevBuf d_desc;                       // kScCells doubles per entry, entry-major
    DevBuf d_labels;                     // int32 per entry
    DevBuf d_jobs;                       // the pending entries' LoopJob
    DevBuf d_counters;                   // k_loop_candidates' two counters (0 between launches)
    LoopCandidate *h_cand = nullptr;     // pinned, host-mapped: the candidate list (h_cap records) and its length
    int64_t *h_count = nullptr;
    size_t h_cap = 0;
    std::vector<int64_t> frames;         // per entry its store frame
    std::vector<int32_t> labels;         // per entry its label
    int64_t described = 0;               // entries [0, described) have their descriptor on the device
    std::vector<LoopJob> jobs;
    bool yaw_guess = false;              // icpmi_loop_set_yaw_guess
    std::vector<int32_t> last_shifts;    // per result of the last detect its shift (-1: the guess was off)
    double gate = 0.0;                   // icpmi_loop_set_gate (0: off)
    std::vector<int64_t> last_pairs;     // per result of the last detect its kept rows (-1: the gate was off)
    int32_t robust_kind = 0;             // icpmi_loop_set_robust (0: off)
    double gicp_epsilon = 0.0;           // icpmi_loop_set_gicp (0: off; never on together with robust_kind)
    double robust_scale = 0.0;
    std::vector<double> last_weights;    // per result of the last detect its weight sum (-1: the weights were off)
    double info_sigma = 0.0, info_floor_r = 0.0, info_floor_t = 0.0;   // icpmi_loop_set_information (sigma 0: off)
    std::vector<double> last_info;       // 36 per result of the last detect (empty: the setting was off)
};

namespace {

void loop_free_host(icpmi_loop *L)
{
    if (L->h_cand) (void)hipHostFree(L->h_cand);
    L->h_cand = nullptr;
    L->h_count = nullptr;
    L->h_cap = 0;
}

// Grow b to hold `bytes`, keeping its first `used` bytes (queued on the stream); the old buffer goes to `old`, to be
// released after the caller's wait.
int loop_grow(icpmi_ctx *ctx, DevBuf &b, size_t used, size_t bytes, std::vector<DevBuf> &old)
{
    if (bytes <= b.cap) return ICPMI_OK;
    DevBuf nb;
    HIP_TRY(ctx, reserve_raw(nb, std::max(bytes, 2 * b.cap)));
    if (used) {
        const hipError_t e = hipMemcpyAsync(nb.p, b.p, used, hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) {
            release(nb);
            return fail(ctx, ICPMI_ERR_HIP, "loop store: %s", hipGetErrorString(e));
        }
    }
    old.push_back(b);
    b = nb;
    return ICPMI_OK;
}

// Queue the descriptors of entries [described, entries): their rows are looked up in the store now (the arena moves
// when it grows, so no device pointer is kept).  The store's own calls end in a wait, so its rows are complete.
int loop_queue_describe(icpmi_loop *L, std::vector<DevBuf> &old)
{
    icpmi_ctx *ctx = L->map->ctx;
    hipStream_t s = ctx->stream;
    const int64_t E = (int64_t)L->frames.size(), e0 = L->described;
    if (e0 >= E) return ICPMI_OK;
    int rc;
    if ((rc = loop_grow(ctx, L->d_desc, sizeof(double) * kScCells * (size_t)e0, sizeof(double) * kScCells * (size_t)E, old)))
        return rc;
    if ((rc = loop_grow(ctx, L->d_labels, sizeof(int32_t) * (size_t)e0, sizeof(int32_t) * (size_t)E, old))) return rc;
    L->jobs.clear();
    for (int64_t e = e0; e < E; ++e) {
        const int64_t f = L->frames[(size_t)e];
        L->jobs.push_back(LoopJob{L->map->row0[(size_t)f], (int32_t)(L->map->row0[(size_t)f + 1] - L->map->row0[(size_t)f]),
                                  L->labels[(size_t)e]});
    }
    if ((rc = reserve(ctx, L->d_jobs, sizeof(LoopJob) * L->jobs.size()))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(L->d_jobs.p, L->jobs.data(), sizeof(LoopJob) * L->jobs.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_loop_describe, dim3((unsigned)(E - e0)), dim3(1024), 0, s, (const double *)L->map->d_rows.p,
                       (const LoopJob *)L->d_jobs.p, (int32_t)e0, (double *)L->d_desc.p, (int32_t *)L->d_labels.p);
    HIP_TRY(ctx, hipGetLastError());
    return ICPMI_OK;
}

// After the wait that ends a call which queued loop_queue_describe: the old buffers go, the entries count as described.
int loop_settle(icpmi_loop *L, std::vector<DevBuf> &old, int rc)
{
    icpmi_ctx *ctx = L->map->ctx;
    if (rc == ICPMI_OK) {
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) L->described = (int64_t)L->frames.size();
        else rc = fail(ctx, ICPMI_ERR_HIP, "loop store: %s", hipGetErrorString(e));
    } else {
        (void)hipStreamSynchronize(ctx->stream); // nothing queued may still read a buffer released below
    }
    for (DevBuf &b : old) release(b);
    old.clear();
    return rc;
}

} // namespace

extern "C" {

void icpmi_loop_config_default(icpmi_loop_config *cfg)
{
    if (!cfg) return;
    cfg->frame_gap = 50;                // loop_closure.hpp:15
    cfg->max_candidates = 3;            // :18
    cfg->sc_distance_threshold = 0.25;  // :16
    cfg->icp_fitness_threshold = 0.3;   // :17
}

int icpmi_loop_create(icpmi_map *map, const icpmi_loop_config *cfg, icpmi_loop **out)
{
    if (!map) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = map->ctx;
    int rc;
    if (!out) return fail(ctx, ICPMI_ERR_NULL, "out is NULL");
    *out = nullptr;
    if ((rc = check_common(ctx))) return rc;
    icpmi_loop *L = new icpmi_loop;
    L->map = map;
    if (cfg) L->cfg = *cfg;
    else icpmi_loop_config_default(&L->cfg);
    hipError_t e = reserve_raw(L->d_counters, 2 * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemsetAsync(L->d_counters.p, 0, 2 * sizeof(unsigned), ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        release(L->d_counters);
        delete L;
        return fail(ctx, ICPMI_ERR_HIP, "loop store: %s", hipGetErrorString(e));
    }
    *out = L;
    return ICPMI_OK;
}

void icpmi_loop_destroy(icpmi_loop *L)
{
    if (!L) return;
    (void)hipSetDevice(L->map->ctx->opt.device);
    (void)hipStreamSynchronize(L->map->ctx->stream);
    for (DevBuf *b : {&L->d_desc, &L->d_labels, &L->d_jobs, &L->d_counters}) release(*b);
    loop_free_host(L);
    delete L;
}

int icpmi_loop_add_frame(icpmi_loop *L, int64_t store_frame, int32_t frame_idx)
{
    if (!L) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = L->map->ctx;
    if (store_frame < 0 || store_frame >= map_frames(L->map))
        return fail(ctx, ICPMI_ERR_ARG, "store frame %lld outside [0, %lld)", (long long)store_frame,
                    (long long)map_frames(L->map));
    if ((int64_t)L->frames.size() >= INT32_MAX) return fail(ctx, ICPMI_ERR_ARG, "too many entries");
    L->frames.push_back(store_frame);
    L->labels.push_back(frame_idx);
    return ICPMI_OK;
}

int icpmi_loop_size(const icpmi_loop *L, int64_t *entries)
{
    if (!L) return ICPMI_ERR_NULL;
    if (entries) *entries = (int64_t)L->frames.size();
    return ICPMI_OK;
}

int icpmi_loop_clear(icpmi_loop *L)
{
    if (!L) return ICPMI_ERR_NULL;
    L->frames.clear();
    L->labels.clear();
    L->described = 0;
    return ICPMI_OK;
}

int icpmi_loop_descriptor(icpmi_loop *L, int64_t entry, double *desc_out)
{
    if (!L) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = L->map->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!desc_out) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (entry < 0 || entry >= (int64_t)L->frames.size())
        return fail(ctx, ICPMI_ERR_ARG, "entry %lld outside [0, %lld)", (long long)entry, (long long)L->frames.size());
    Range range("icpmi:loop_descriptor");
    std::vector<DevBuf> old;
    rc = loop_queue_describe(L, old);
    if (rc == ICPMI_OK) {
        const hipError_t e = hipMemcpyAsync(desc_out, (const double *)L->d_desc.p + (size_t)entry * kScCells,
                                            sizeof(double) * kScCells, hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) rc = fail(ctx, ICPMI_ERR_HIP, "loop store: %s", hipGetErrorString(e));
    }
    return loop_settle(L, old, rc); // the call's one wait
}

int icpmi_loop_detect(icpmi_loop *L, icpmi_loop_result *out, int64_t cap, int64_t *n_out)
{
    if (!L) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = L->map->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!n_out || (!out && cap > 0)) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    if (ctx->comm || ctx->cb_allreduce) return fail(ctx, ICPMI_ERR_ARG, "a context with a communicator registers one (sharded) problem at a time");
    *n_out = 0;
    L->last_shifts.clear();
    L->last_pairs.clear();
    L->last_weights.clear();
    L->last_info.clear();
    const bool guess = L->yaw_guess;
    const bool gated = L->gate > 0.0;
    const int32_t robust = L->robust_kind;
    const double robust_ks = robust == ICPMI_ROBUST_GEMAN_MCCLURE ? L->robust_scale * L->robust_scale : L->robust_scale;
    const bool gicp = L->gicp_epsilon > 0.0; // (plane-to-plane verifications: the small form, behind the loop's gate)
    const icpmi_gicp gicp_rule{L->gicp_epsilon, gated ? L->gate : 0.0, ICPMI_GICP_FORM_SMALL};
    const int64_t E = (int64_t)L->frames.size();
    if (E < 2) return ICPMI_OK; // :69
    Range range("icpmi:loop_detect");
    hipStream_t s = ctx->stream;
    const int64_t q = E - 1;
    std::vector<DevBuf> old;
    rc = loop_queue_describe(L, old);
    if (rc == ICPMI_OK && (size_t)q > L->h_cap) { // the list holds every older entry, at worst
        loop_free_host(L);
        const size_t cap_rec = std::max<size_t>(2 * (size_t)q, 1024);
        void *h = nullptr;
        const hipError_t e = hipHostMalloc(&h, sizeof(LoopCandidate) * cap_rec + 64, hipHostMallocMapped);
        if (e != hipSuccess) rc = fail(ctx, ICPMI_ERR_HIP, "loop store: hipHostMalloc: %s", hipGetErrorString(e));
        else {
            L->h_cand = (LoopCandidate *)h;
            L->h_count = (int64_t *)((char *)h + sizeof(LoopCandidate) * cap_rec);
            L->h_cap = cap_rec;
        }
    }
    LoopCandidate *d_cand = nullptr;
    int64_t *d_count = nullptr;
    if (rc == ICPMI_OK) {
        hipError_t e = hipHostGetDevicePointer((void **)&d_cand, L->h_cand, 0);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&d_count, L->h_count, 0);
        if (e != hipSuccess) rc = fail(ctx, ICPMI_ERR_HIP, "loop store: hipHostGetDevicePointer: %s", hipGetErrorString(e));
    }
    if (rc == ICPMI_OK) {
        *L->h_count = -1;
        if (guess)
            hipLaunchKernelGGL(k_loop_candidates_shift, dim3((unsigned)q), dim3(64), 0, s, (const double *)L->d_desc.p,
                               (const int32_t *)L->d_labels.p, (int32_t)q, L->cfg.frame_gap, L->cfg.sc_distance_threshold,
                               (unsigned *)L->d_counters.p, (LoopCandidateShift *)d_cand, d_count);
        else
            hipLaunchKernelGGL(k_loop_candidates, dim3((unsigned)q), dim3(64), 0, s, (const double *)L->d_desc.p,
                               (const int32_t *)L->d_labels.p, (int32_t)q, L->cfg.frame_gap, L->cfg.sc_distance_threshold,
                               (unsigned *)L->d_counters.p, d_cand, d_count);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = fail(ctx, ICPMI_ERR_HIP, "k_loop_candidates: %s", hipGetErrorString(e));
    }
    if ((rc = loop_settle(L, old, rc))) return rc; // the call's one wait before the verifications
    const int64_t nc = *(volatile int64_t *)L->h_count;
    if (nc < 0 || nc > q) return fail(ctx, ICPMI_ERR_HIP, "k_loop_candidates returned %lld candidates of %lld", (long long)nc, (long long)q);
    std::vector<std::pair<double, int>> candidates;
    candidates.reserve((size_t)nc);
    std::vector<int32_t> shift_of; // per entry its shift (guess only): it rides along and never enters the order
    if (guess) {
        shift_of.assign((size_t)q, 0);
        const LoopCandidateShift *h = (const LoopCandidateShift *)L->h_cand;
        for (int64_t i = 0; i < nc; ++i) {
            if (h[i].entry < 0 || h[i].entry >= q || h[i].shift < 0 || h[i].shift >= kScSectors)
                return fail(ctx, ICPMI_ERR_HIP, "k_loop_candidates_shift returned entry %d, shift %d", h[i].entry, h[i].shift);
            candidates.emplace_back(h[i].dist, (int)h[i].entry);
            shift_of[(size_t)h[i].entry] = h[i].shift;
        }
    } else {
        for (int64_t i = 0; i < nc; ++i) candidates.emplace_back(L->h_cand[i].dist, (int)L->h_cand[i].entry);
    }
    std::sort(candidates.begin(), candidates.end()); // :93

    // :96-123: verify in order until max_candidates are accepted; the next min(max_candidates - accepted,
    // ICPMI_MAX_BATCH) run side by side on the batch's helper contexts, straight from the store
    icpmi_config icp;
    icpmi_config_default(&icp);
    icp.max_iterations = 30; // :102-105
    icp.tolerance = 1e-6;
    const int32_t hcap = icp.max_iterations + 1;
    std::vector<icpmi_loop_result> results;
    const double *rows = (const double *)L->map->d_rows.p;
    const int64_t fq = L->frames[(size_t)q];
    const int64_t q0 = L->map->row0[(size_t)fq], nq = L->map->row0[(size_t)fq + 1] - q0;
    int verified = 0;
    size_t pos = 0;
    while (pos < candidates.size() && verified < L->cfg.max_candidates) { // :97
        const int32_t take = (int32_t)std::min<size_t>(candidates.size() - pos,
                                                       std::min<size_t>((size_t)(L->cfg.max_candidates - verified), ICPMI_MAX_BATCH));
        icpmi_result res[ICPMI_MAX_BATCH];
        int32_t status[ICPMI_MAX_BATCH];
        std::vector<double> hist((size_t)take * (size_t)hcap);
        icpmi_config icps[ICPMI_MAX_BATCH]; // every problem its own start
        GateRun gates[ICPMI_MAX_BATCH];
        for (int32_t k = 0; k < take; ++k) {
            icps[k] = icp;
            if (guess && (rc = icpmi_sc_shift_transform(shift_of[(size_t)candidates[pos + (size_t)k].second], icps[k].initial_transform)))
                return fail(ctx, rc, "internal: shift out of range");
        }
        rc = batch_run(ctx, take, [&](icpmi_ctx *c, int k) {
            const int64_t f = L->frames[(size_t)candidates[pos + (size_t)k].second];
            const int64_t t0 = L->map->row0[(size_t)f], nt = L->map->row0[(size_t)f + 1] - t0;
            // (only the sizes are checked: the rows are the store's, non-null even for a frame of 0 rows)
            int r = validate_align(c, &icp, nq, &icp, nt, &icps[k], &res[k], hist.data() + (size_t)k * hcap, hcap);
            if (r == ICPMI_OK) r = check_common(c);
            gates[k] = GateRun{L->gate * L->gate, 0};
            if (robust) gates[k] = GateRun{gated ? L->gate * L->gate : 1.7976931348623157e308, 0, robust, robust_ks, 0.0};
            if (gicp && r == ICPMI_OK) r = validate_gicp(c, &gicp_rule, &gates[k]);
            if (r == ICPMI_OK)
                r = align_staged(c, rows + 3 * (size_t)q0, nq, rows + 3 * (size_t)t0, nt, hipMemcpyDeviceToDevice, &icps[k],
                                 &res[k], hist.data() + (size_t)k * hcap, hcap, gated || robust || gicp ? &gates[k] : nullptr);
            return r;
        }, status);
        if (rc) return rc;
        for (int32_t k = 0; k < take; ++k) {
            const icpmi_result &r = res[k];
            const auto &cand = candidates[pos + (size_t)k];
            if (r.converged && r.final_error < L->cfg.icp_fitness_threshold) { // :112
                icpmi_loop_result o;
                o.query_frame = L->labels[(size_t)q];
                o.match_frame = L->labels[(size_t)cand.second];
                memcpy(o.transform, r.transformation, sizeof(o.transform));
                o.scan_context_distance = cand.first;
                o.icp_fitness = r.final_error;
                results.push_back(o);
                L->last_shifts.push_back(guess ? shift_of[(size_t)cand.second] : -1);
                L->last_pairs.push_back(gated || gicp ? gates[k].pairs : -1);
                L->last_weights.push_back(robust ? gates[k].weight_sum : -1.0);
                if (L->info_sigma > 0.0) { // the verification's own normal matrix, on the context that ran it
                    icpmi_normal_matrix nm;
                    double info[36];
                    if ((rc = icpmi_last_normal_matrix(ctx, k, &nm))) return rc;
                    if ((rc = icpmi_information_from_icp(nm.JtJ, nm.T, L->info_sigma, L->info_floor_r, L->info_floor_t, info)))
                        return fail(ctx, rc, "loop store: the information of an accepted closure is not finite");
                    L->last_info.insert(L->last_info.end(), info, info + 36);
                }
                ++verified;
            }
        }
        pos += (size_t)take;
    }
    *n_out = (int64_t)results.size();
    if ((int64_t)results.size() > cap)
        return fail(ctx, ICPMI_ERR_CAPACITY, "output holds %lld results, needs %lld", (long long)cap, (long long)results.size());
    if (!results.empty()) memcpy(out, results.data(), sizeof(icpmi_loop_result) * results.size());
    return ICPMI_OK;
}

int icpmi_loop_set_yaw_guess(icpmi_loop *L, int32_t on)
{
    if (!L) return ICPMI_ERR_NULL;
    L->yaw_guess = on != 0;
    return ICPMI_OK;
}

int icpmi_loop_set_gate(icpmi_loop *L, double max_distance)
{
    if (!L) return ICPMI_ERR_NULL;
    if (max_distance != 0.0 && (!(max_distance > 0.0) || !std::isfinite(max_distance)))
        return fail(L->map->ctx, ICPMI_ERR_ARG, "max_distance must be 0 (off) or finite and > 0");
    L->gate = max_distance;
    return ICPMI_OK;
}

int icpmi_loop_set_robust(icpmi_loop *L, int32_t kind, double scale)
{
    if (!L) return ICPMI_ERR_NULL;
    if (kind == 0) {
        L->robust_kind = 0;
        L->robust_scale = 0.0;
        return ICPMI_OK;
    }
    if (kind != ICPMI_ROBUST_HUBER && kind != ICPMI_ROBUST_GEMAN_MCCLURE)
        return fail(L->map->ctx, ICPMI_ERR_ARG, "kind %d is neither 0 (off), ICPMI_ROBUST_HUBER nor ICPMI_ROBUST_GEMAN_MCCLURE", (int)kind);
    if (!(scale > 0.0) || !std::isfinite(scale)) return fail(L->map->ctx, ICPMI_ERR_ARG, "scale must be finite and > 0");
    if (L->gicp_epsilon > 0.0) return fail(L->map->ctx, ICPMI_ERR_ARG, "plane-to-plane verifications take no robust weights (icpmi_loop_set_gicp(0) first)");
    L->robust_kind = kind;
    L->robust_scale = scale;
    return ICPMI_OK;
}

int icpmi_loop_set_gicp(icpmi_loop *L, double epsilon)
{
    if (!L) return ICPMI_ERR_NULL;
    if (epsilon == 0.0) {
        L->gicp_epsilon = 0.0;
        return ICPMI_OK;
    }
    if (!(epsilon > 0.0 && epsilon <= 1.0)) return fail(L->map->ctx, ICPMI_ERR_ARG, "epsilon must be 0 (off) or finite with 0 < epsilon <= 1");
    if (L->robust_kind != 0) return fail(L->map->ctx, ICPMI_ERR_ARG, "plane-to-plane verifications take no robust weights (icpmi_loop_set_robust(0, 0) first)");
    L->gicp_epsilon = epsilon;
    return ICPMI_OK;
}

int icpmi_loop_set_information(icpmi_loop *L, double sigma, double floor_rotation_sigma, double floor_translation_sigma)
{
    if (!L) return ICPMI_ERR_NULL;
    if (sigma == 0.0) {
        L->info_sigma = L->info_floor_r = L->info_floor_t = 0.0;
        return ICPMI_OK;
    }
    const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    double zero[36] = {0.0}, out[36];
    if (icpmi_information_from_icp(zero, eye, sigma, floor_rotation_sigma, floor_translation_sigma, out) != ICPMI_OK)
        return fail(L->map->ctx, ICPMI_ERR_ARG, "sigma must be 0 (off) or finite and > 0, a floor 0 or finite and > 0");
    L->info_sigma = sigma;
    L->info_floor_r = floor_rotation_sigma;
    L->info_floor_t = floor_translation_sigma;
    return ICPMI_OK;
}

int icpmi_loop_last_information(const icpmi_loop *L, double *info, int64_t cap, int64_t *n_out)
{
    if (!L) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = L->map->ctx;
    if (!n_out || (!info && cap > 0)) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    const int64_t n = (int64_t)L->last_info.size() / 36;
    *n_out = n;
    if (n > cap) return fail(ctx, ICPMI_ERR_CAPACITY, "output holds %lld matrices, needs %lld", (long long)cap, (long long)n);
    if (n) memcpy(info, L->last_info.data(), sizeof(double) * 36 * (size_t)n);
    return ICPMI_OK;
}

int icpmi_loop_last_weights(const icpmi_loop *L, double *weights, int64_t cap, int64_t *n_out)
{
    if (!L) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = L->map->ctx;
    if (!n_out || (!weights && cap > 0)) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    const int64_t n = (int64_t)L->last_weights.size();
    *n_out = n;
    if (n > cap) return fail(ctx, ICPMI_ERR_CAPACITY, "output holds %lld weights, needs %lld", (long long)cap, (long long)n);
    if (n) memcpy(weights, L->last_weights.data(), sizeof(double) * (size_t)n);
    return ICPMI_OK;
}

int icpmi_loop_last_pairs(const icpmi_loop *L, int64_t *pairs, int64_t cap, int64_t *n_out)
{
    if (!L) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = L->map->ctx;
    if (!n_out || (!pairs && cap > 0)) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    const int64_t n = (int64_t)L->last_pairs.size();
    *n_out = n;
    if (n > cap) return fail(ctx, ICPMI_ERR_CAPACITY, "output holds %lld counts, needs %lld", (long long)cap, (long long)n);
    if (n) memcpy(pairs, L->last_pairs.data(), sizeof(int64_t) * (size_t)n);
    return ICPMI_OK;
}

int icpmi_loop_last_shifts(const icpmi_loop *L, int32_t *shifts, int64_t cap, int64_t *n_out)
{
    if (!L) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = L->map->ctx;
    if (!n_out || (!shifts && cap > 0)) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    const int64_t n = (int64_t)L->last_shifts.size();
    *n_out = n;
    if (n > cap) return fail(ctx, ICPMI_ERR_CAPACITY, "output holds %lld shifts, needs %lld", (long long)cap, (long long)n);
    if (n) memcpy(shifts, L->last_shifts.data(), sizeof(int32_t) * (size_t)n);
    return ICPMI_OK;
}

} // extern "C"

// ======================================================================================================================
// Local map (local_map.h): the sliding voxel table scan-to-local-map odometry registers against.  Two buffers of
// `capacity` rows each (keys, points); an add reads the current one and writes the other, and they change places once
// the add's one wait has shown that the result fits.

struct icpmi_local_map {
    icpmi_ctx *ctx = nullptr;
    icpmi_local_map_config cfg{};
    DevBuf d_keys[2], d_pts[2];          // the table and the buffer the next add writes
    int cur = 0;                         // which of the two is the table
    int64_t rows = 0;
    DevBuf d_scan, d_world;              // a host add's rows on the device; the scan's world points
    DevBuf d_new_keys, d_new_vals;       // keys in | sorted ; rows in | sorted
    DevBuf d_marks;                      // marks (rows + n + 1) | their exclusive sum ; then the words read back
    unsigned *h_words = nullptr;         // pinned: surviving residents, rows of the new table, dropped rows
};

namespace {

constexpr int64_t kLmapMaxRows = (int64_t)1 << 27;

const double *lmap_points(const icpmi_local_map *m) { return (const double *)m->d_pts[m->cur].p; }

// a table change: a target remembered at either buffer's address is no longer what the context's buffers describe
void lmap_forget_target(icpmi_local_map *m)
{
    icpmi_ctx *ctx = m->ctx;
    if (ctx->tgt.prep_tgt == (const double *)m->d_pts[0].p || ctx->tgt.prep_tgt == (const double *)m->d_pts[1].p) ctx->tgt.prep_valid = false;
}

// d_scan: n rows in device memory (null with n == 0)
int lmap_add(icpmi_local_map *m, const double *d_scan, int64_t n64, const double pose[16], icpmi_local_map_info *info)
{
    icpmi_ctx *ctx = m->ctx;
    hipStream_t s = ctx->stream;
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(pose[i])) return fail(ctx, ICPMI_ERR_ARG, "pose entry %d is not finite", i);
    if (n64 < 0 || n64 > kLmapMaxRows) return fail(ctx, ICPMI_ERR_ARG, "n = %lld outside [0, 2^27]", (long long)n64);
    Range range("icpmi:local_map_add");
    const unsigned n = (unsigned)n64, R = (unsigned)m->rows;
    const size_t un = n, elems = (size_t)R + un + 1;
    int rc;
    if ((rc = reserve(ctx, m->d_world, sizeof(double) * 3 * un))) return rc;
    if ((rc = reserve(ctx, m->d_new_keys, sizeof(unsigned long long) * 2 * un))) return rc;
    if ((rc = reserve(ctx, m->d_new_vals, sizeof(unsigned) * 2 * un))) return rc;
    if ((rc = reserve(ctx, m->d_marks, sizeof(unsigned) * (2 * elems + 4)))) return rc;
    unsigned long long *keys_in = (unsigned long long *)m->d_new_keys.p, *keys = keys_in + un;
    unsigned *vals_in = (unsigned *)m->d_new_vals.p, *order = vals_in + un;
    unsigned *marks = (unsigned *)m->d_marks.p, *offs = marks + elems, *words = marks + 2 * elems;
    size_t b1 = 0, b2 = 0;
    if (n) HIP_TRY(ctx, sort_pairs_u64_all(nullptr, &b1, keys_in, keys, vals_in, order, n, s));
    HIP_TRY(ctx, exclusive_sum_u32(nullptr, &b2, marks, offs, (unsigned)elems, s));
    if ((rc = reserve(ctx, ctx->sort_tmp, std::max(b1, b2)))) return rc;

    const double r2 = m->cfg.max_range * m->cfg.max_range;
    const unsigned long long *res_keys = (const unsigned long long *)m->d_keys[m->cur].p;
    const double *res_pts = lmap_points(m);
    const int nxt = m->cur ^ 1;
    HIP_TRY(ctx, hipMemsetAsync(words, 0, 4 * sizeof(unsigned), s));
    if (n) {
        Rigid34 P{pose[0], pose[1], pose[2], pose[3], pose[4], pose[5], pose[6], pose[7], pose[8], pose[9], pose[10], pose[11]};
        hipLaunchKernelGGL(k_lmap_keys, dim3(lmap_blocks(un)), dim3(256), 0, s, d_scan, n, P, m->cfg.voxel_size, r2,
                           (double *)m->d_world.p, keys_in, vals_in, words);
        HIP_TRY(ctx, sort_pairs_u64_all(ctx->sort_tmp.p, &b1, keys_in, keys, vals_in, order, n, s));
    }
    hipLaunchKernelGGL(k_lmap_marks, dim3(lmap_blocks(elems)), dim3(256), 0, s, res_keys, res_pts, R, (const unsigned long long *)keys, n,
                       pose[3], pose[7], pose[11], r2, marks);
    HIP_TRY(ctx, exclusive_sum_u32(ctx->sort_tmp.p, &b2, marks, offs, (unsigned)elems, s));
    hipLaunchKernelGGL(k_lmap_merge, dim3(lmap_blocks(elems)), dim3(256), 0, s, res_keys, res_pts, R, (const unsigned long long *)keys,
                       (const unsigned *)order, (const double *)m->d_world.p, n, (const unsigned *)marks, (const unsigned *)offs,
                       (unsigned long long)m->cfg.capacity, (unsigned long long *)m->d_keys[nxt].p, (double *)m->d_pts[nxt].p, words);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(m->h_words, words, 4 * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s)); // the call's one wait
    const int64_t S = m->h_words[kLmapS], total = m->h_words[kLmapTotal], dropped = m->h_words[kLmapDroppedRows];
    if (total > m->cfg.capacity)
        return fail(ctx, ICPMI_ERR_CAPACITY, "the add would leave %lld rows; the local map holds %lld", (long long)total,
                    (long long)m->cfg.capacity);
    lmap_forget_target(m);
    m->cur = nxt;
    m->rows = total;
    if (info) {
        info->rows = total;
        info->inserted = total - S;
        info->evicted = (int64_t)R - S;
        info->dropped = dropped;
        info->merged = n64 - info->inserted - dropped;
    }
    // the new table as the next registration's target, queued and not waited for (a failure only means that
    // the registration prepares it itself: it must not leave its text in the error string of an add that succeeded)
    if (total > 0 && !ctx->comm && !ctx->cb_allreduce) {
        const std::string keep = ctx->err;
        if (prepare_target(ctx, lmap_points(m), (int)total, (int)n) != ICPMI_OK) {
            ctx->err = keep;
            ctx->tgt.prep_valid = false;
        }
        ctx->trailing_work = true;
    }
    return ICPMI_OK;
}

int lmap_check(icpmi_local_map *m, const double *pose)
{
    int rc;
    if ((rc = check_common(m->ctx))) return rc;
    if (!pose) return fail(m->ctx, ICPMI_ERR_NULL, "pose is NULL");
    return ICPMI_OK;
}

// the scan in host memory -> the handle's staging rows
int lmap_stage(icpmi_local_map *m, const double *xyz, int64_t n)
{
    icpmi_ctx *ctx = m->ctx;
    int rc;
    if (n < 0 || n > kLmapMaxRows) return fail(ctx, ICPMI_ERR_ARG, "n = %lld outside [0, 2^27]", (long long)n);
    if ((rc = reserve(ctx, m->d_scan, sizeof(double) * 3 * (size_t)n))) return rc;
    if (n) HIP_TRY(ctx, hipMemcpyAsync(m->d_scan.p, xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    return ICPMI_OK;
}

// registration of n rows (device memory) against the table; rule: null for the plain one
int lmap_register(icpmi_local_map *m, const double *d_xyz, int64_t n, const icpmi_config *cfg, const icpmi_robust *rule,
                  icpmi_result *result, icpmi_robust_info *info, double *error_history, int32_t history_cap)
{
    icpmi_ctx *ctx = m->ctx;
    if (rule)
        return icpmi_align_robust_device(ctx, d_xyz, n, lmap_points(m), m->rows, cfg, rule, result, info, error_history, history_cap);
    return icpmi_align_device(ctx, d_xyz, n, lmap_points(m), m->rows, cfg, result, error_history, history_cap);
}

int lmap_register_host(icpmi_local_map *m, const double *xyz, int64_t n, const icpmi_config *cfg, const icpmi_robust *rule,
                       bool robust, icpmi_result *result, icpmi_robust_info *info, double *error_history, int32_t history_cap)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    int rc = validate_align(ctx, xyz, n, lmap_points(m), m->rows, cfg, result, error_history, history_cap);
    if (rc) return rc;
    if (robust && !rule) return fail(ctx, ICPMI_ERR_NULL, "rule is NULL (no weights: icpmi_local_map_register)");
    if ((rc = check_common(ctx))) return rc;
    if ((rc = reserve(ctx, ctx->stage_b, sizeof(double) * 3 * (size_t)n))) return rc; // where icpmi_align puts its source
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stage_b.p, xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    return lmap_register(m, (const double *)ctx->stage_b.p, n, cfg, rule, result, info, error_history, history_cap);
}

} // namespace

extern "C" {

void icpmi_local_map_config_default(icpmi_local_map_config *cfg)
{
    if (!cfg) return;
    cfg->voxel_size = 0.5;
    cfg->max_range = 100.0;
    cfg->capacity = (int64_t)1 << 20;
}

int icpmi_local_map_create(icpmi_ctx *ctx, const icpmi_local_map_config *cfg, icpmi_local_map **out)
{
    int rc;
    if (!out) return fail(ctx, ICPMI_ERR_NULL, "out is NULL");
    *out = nullptr;
    if ((rc = check_common(ctx))) return rc;
    if (!cfg) return fail(ctx, ICPMI_ERR_NULL, "cfg is NULL");
    if (!(cfg->voxel_size > 0.0) || !std::isfinite(cfg->voxel_size)) return fail(ctx, ICPMI_ERR_ARG, "voxel_size must be finite and > 0");
    if (!(cfg->max_range > 0.0) || !std::isfinite(cfg->max_range)) return fail(ctx, ICPMI_ERR_ARG, "max_range must be finite and > 0");
    if (cfg->capacity < 1 || cfg->capacity > kLmapMaxRows) return fail(ctx, ICPMI_ERR_ARG, "capacity outside [1, 2^27]");
    icpmi_local_map *m = new icpmi_local_map;
    m->ctx = ctx;
    m->cfg = *cfg;
    hipError_t e = hipHostMalloc((void **)&m->h_words, 4 * sizeof(unsigned), hipHostMallocDefault);
    for (int b = 0; b < 2 && e == hipSuccess; ++b) {
        if ((e = hipMalloc(&m->d_keys[b].p, sizeof(unsigned long long) * (size_t)cfg->capacity)) == hipSuccess)
            m->d_keys[b].cap = sizeof(unsigned long long) * (size_t)cfg->capacity;
        if (e == hipSuccess && (e = hipMalloc(&m->d_pts[b].p, sizeof(double) * 3 * (size_t)cfg->capacity)) == hipSuccess)
            m->d_pts[b].cap = sizeof(double) * 3 * (size_t)cfg->capacity;
    }
    if (e != hipSuccess) {
        icpmi_local_map_destroy(m);
        return fail(ctx, ICPMI_ERR_HIP, "local map of %lld rows: %s", (long long)cfg->capacity, hipGetErrorString(e));
    }
    *out = m;
    return ICPMI_OK;
}

void icpmi_local_map_destroy(icpmi_local_map *m)
{
    if (!m) return;
    (void)hipSetDevice(m->ctx->opt.device);
    (void)hipStreamSynchronize(m->ctx->stream);
    lmap_forget_target(m);
    for (DevBuf *b : {&m->d_keys[0], &m->d_keys[1], &m->d_pts[0], &m->d_pts[1], &m->d_scan, &m->d_world, &m->d_new_keys,
                      &m->d_new_vals, &m->d_marks})
        release(*b);
    if (m->h_words) (void)hipHostFree(m->h_words);
    delete m;
}

int icpmi_local_map_clear(icpmi_local_map *m)
{
    if (!m) return ICPMI_ERR_NULL;
    int rc;
    if ((rc = check_common(m->ctx))) return rc;
    lmap_forget_target(m);
    m->rows = 0;
    return ICPMI_OK;
}

int icpmi_local_map_add(icpmi_local_map *m, const double *xyz, int64_t n, const double pose[16], icpmi_local_map_info *info)
{
    if (!m) return ICPMI_ERR_NULL;
    int rc;
    if ((rc = lmap_check(m, pose))) return rc;
    if (!xyz && n != 0) return fail(m->ctx, ICPMI_ERR_NULL, "null argument");
    if ((rc = lmap_stage(m, xyz, n))) return rc;
    return lmap_add(m, (const double *)m->d_scan.p, n, pose, info);
}

int icpmi_local_map_add_device(icpmi_local_map *m, const double *d_xyz, int64_t n, const double pose[16], icpmi_local_map_info *info)
{
    if (!m) return ICPMI_ERR_NULL;
    int rc;
    if ((rc = lmap_check(m, pose))) return rc;
    if (!d_xyz && n != 0) return fail(m->ctx, ICPMI_ERR_NULL, "null argument");
    return lmap_add(m, d_xyz, n, pose, info);
}

int icpmi_local_map_add_stream_frame(icpmi_local_map *m, const double pose[16], icpmi_local_map_info *info)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    int rc;
    if ((rc = lmap_check(m, pose))) return rc;
    if (ctx->stream_prev_n < 0) return fail(ctx, ICPMI_ERR_ARG, "no resident frame: call icpmi_stream_push first");
    return lmap_add(m, (const double *)ctx->stream_prev.p, ctx->stream_prev_n, pose, info);
}

int icpmi_local_map_size(const icpmi_local_map *m, int64_t *rows)
{
    if (!m) return ICPMI_ERR_NULL;
    if (!rows) return fail(m->ctx, ICPMI_ERR_NULL, "rows is NULL");
    *rows = m->rows;
    return ICPMI_OK;
}

int icpmi_local_map_points(icpmi_local_map *m, double *out_xyz, uint64_t *out_keys, int64_t cap, int64_t *n_out)
{
    if (!m) return ICPMI_ERR_NULL;
    icpmi_ctx *ctx = m->ctx;
    int rc;
    if ((rc = check_common(ctx))) return rc;
    if (!n_out) return fail(ctx, ICPMI_ERR_NULL, "null argument");
    *n_out = m->rows;
    if ((!out_xyz && !out_keys) || m->rows == 0) return ICPMI_OK;
    if (cap < m->rows) return fail(ctx, ICPMI_ERR_CAPACITY, "output holds %lld rows, needs %lld", (long long)cap, (long long)m->rows);
    if (out_xyz) HIP_TRY(ctx, hipMemcpyAsync(out_xyz, lmap_points(m), sizeof(double) * 3 * (size_t)m->rows, hipMemcpyDeviceToHost, ctx->stream));
    if (out_keys) HIP_TRY(ctx, hipMemcpyAsync(out_keys, m->d_keys[m->cur].p, sizeof(uint64_t) * (size_t)m->rows, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ICPMI_OK;
}

int icpmi_local_map_register(icpmi_local_map *m, const double *xyz, int64_t n, const icpmi_config *cfg, icpmi_result *result,
                             double *error_history, int32_t history_cap)
{
    return lmap_register_host(m, xyz, n, cfg, nullptr, false, result, nullptr, error_history, history_cap);
}

int icpmi_local_map_register_device(icpmi_local_map *m, const double *d_xyz, int64_t n, const icpmi_config *cfg, icpmi_result *result,
                                    double *error_history, int32_t history_cap)
{
    if (!m) return ICPMI_ERR_NULL;
    return lmap_register(m, d_xyz, n, cfg, nullptr, result, nullptr, error_history, history_cap);
}

int icpmi_local_map_register_robust(icpmi_local_map *m, const double *xyz, int64_t n, const icpmi_config *cfg, const icpmi_robust *rule,
                                    icpmi_result *result, icpmi_robust_info *info, double *error_history, int32_t history_cap)
{
    return lmap_register_host(m, xyz, n, cfg, rule, true, result, info, error_history, history_cap);
}

int icpmi_local_map_register_robust_device(icpmi_local_map *m, const double *d_xyz, int64_t n, const icpmi_config *cfg,
                                           const icpmi_robust *rule, icpmi_result *result, icpmi_robust_info *info,
                                           double *error_history, int32_t history_cap)
{
    if (!m) return ICPMI_ERR_NULL;
    if (!rule) return fail(m->ctx, ICPMI_ERR_NULL, "rule is NULL (no weights: icpmi_local_map_register_device)");
    return lmap_register(m, d_xyz, n, cfg, rule, result, info, error_history, history_cap);
}

} // extern "C"
