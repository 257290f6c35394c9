/*
 * icp_mi355x.h -- C ABI of libicp_mi355x.so: point-to-plane ICP registration on one
 * MI355X (gfx950), optionally source-sharded over several with RCCL.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference has no
 * FFI layer; its boundary is the header-only C++ function
 *     slam::icp_point_to_plane(const PointCloud&, const PointCloud&, const ICPConfig&)
 *         -> ICPResult                      (slam_viz/core/icp.hpp:157-161)
 * called from slam_node.cpp:138 and loop_closure.hpp:109.  Each entry point below
 * names the reference interface it replaces (paths relative to
 * slam_viz/include/slam_viz/core/).  Plain pointers and sizes only.
 *
 * Conventions
 *   - points: row-major N x 3 fp64, contiguous ("xyzxyz...", types.hpp:17).
 *   - 4x4 transforms: ROW-major double[16] here.  Eigen::Matrix4d is column-major
 *     (types.hpp:76); an adapter must convert element-wise, never memcpy.
 *   - every function returns ICPMI_OK (0) or a negative ICPMI_ERR_* code; the text
 *     of the last failure is available from icpmi_last_error().
 *   - one icpmi_ctx serves one caller thread at a time; distinct contexts may run
 *     concurrently.  Calls block until results are on the host.
 *   - stream ordering of the *_device entry points: the library works on a private
 *     non-blocking HIP stream that is NOT ordered against any stream of the caller
 *     (torch's current stream included).  Device inputs must be complete and visible
 *     before the call (synchronise the producing stream, or wait on its event, first);
 *     device outputs are complete when the call returns.  One exception in what "returns" means:
 *     icpmi_stream_push* hand back their RESULTS complete, but may leave kernels of the library's own
 *     queued on that stream -- the search structure and normals of the scan just filtered, the next
 *     push's target -- so that the device builds them while the caller digests the result.  They touch
 *     only the context's workspace; every later call on the context is ordered behind them, and a
 *     fault in them is reported by that next call as a failure of the preparation step.
 *   - there is no CPU fallback: with no usable HIP device icpmi_create fails.
 */
#ifndef ICP_MI355X_H
#define ICP_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICPMI_OK 0
#define ICPMI_ERR_NULL (-1)          /* a required pointer is NULL */
#define ICPMI_ERR_EMPTY_SOURCE (-2)  /* n_src <= 0 (reference: division by zero, icp.hpp:206) */
#define ICPMI_ERR_EMPTY_TARGET (-3)  /* n_tgt <= 0 (reference: row(-1) UB, kdtree.hpp:33-36,211) */
#define ICPMI_ERR_CAPACITY (-4)      /* error_history buffer smaller than max_iterations + 1 */
#define ICPMI_ERR_HIP (-5)           /* HIP runtime failure */
#define ICPMI_ERR_RCCL (-6)          /* RCCL failure */
#define ICPMI_ERR_ARG (-7)           /* argument out of range */
#define ICPMI_ERR_NO_DEVICE (-8)     /* no gfx950 device / kernels not loadable */

/* nearest-neighbour search engines (all return the exact fp64 nearest neighbour) */
#define ICPMI_SEARCH_AUTO 0
#define ICPMI_SEARCH_EXACT_F64 1     /* fp64 brute force, SGPR-broadcast targets */
#define ICPMI_SEARCH_MFMA_BF16 2     /* bf16 MFMA coarse pass over ALL pairs + certified fp64 resolve.  "All pairs" names
                                        the coarse pass of the ICP loop (and of the stand-alone searches): the k-NN setup
                                        of a target -- its 20-NN among itself, for the normals -- is culled like engine
                                        3's on targets of more than 12 splits (24,576 points) in both MFMA engines, with
                                        the same lists and normals bit for bit; ICPMI_KNN_CULL=0 in the environment keeps
                                        that setup on all pairs too */
#define ICPMI_SEARCH_MFMA_PRUNED 3   /* the same, skipping (32-row tile, target split) pairs whose bounding
                                        boxes are farther apart than the tile's known neighbour distance -- the
                                        rule of kdtree.hpp:139,177 applied to groups; same exact result, not an
                                        all-pairs pass (registrations and normal estimation).  AUTO takes it for
                                        targets of more than 12 splits (24,576 points), engine 2 below that; targets
                                        of more than 3,072 splits (6.29M points) or sources of 2^25 rows and more
                                        run on engine 2 whichever of the two was asked for */

typedef struct icpmi_ctx icpmi_ctx;

typedef struct {
    int32_t device;     /* HIP device ordinal */
    int32_t normal_k;   /* neighbours for PCA normals; the reference hard-codes 20 (icp.hpp:170) */
    int32_t search;     /* ICPMI_SEARCH_* */
    int32_t profile;    /* 0 off; 1: HIP events around the call, the loop and every 4th launch of the
                           dominant kernel; 2: around every stage (icpmi_get_profile) */
} icpmi_options;

/* mirrors slam::ICPConfig, types.hpp:143-148 */
typedef struct {
    int32_t max_iterations;        /* default 50 */
    int32_t reserved;
    double tolerance;              /* default 1e-6 */
    double min_error;              /* default 1e-9 */
    double initial_transform[16];  /* row-major, default identity */
} icpmi_config;

/* mirrors slam::ICPResult, types.hpp:155-164 */
typedef struct {
    double transformation[16];     /* row-major, maps source -> target (icp.hpp:154-155) */
    int32_t converged;
    int32_t num_iterations;        /* error_history.size() - 1 (icp.hpp:255) */
    double final_error;
    int32_t history_len;           /* entries written to error_history */
    int32_t loop_iterations;       /* loop bodies entered (not a reference field) */
} icpmi_result;

/* per-stage device time from HIP events on the library's stream, accumulated since
 * the last icpmi_reset_profile(); only filled when options.profile != 0 */
typedef struct {
    double nn_ms;        int64_t nn_launches;        /* correspondence search passes (coarse + resolve) */
    double coarse_ms;    int64_t coarse_launches;    /* k_nn_coarse alone: the dominant kernel (the launches bracketed) */
    double reduce_ms;    int64_t reduce_launches;    /* residual + 6x6 accumulation + solve */
    double transform_ms; int64_t transform_launches;
    double normals_ms;   int64_t normals_launches;   /* k-NN + PCA */
    double total_ms;     int64_t calls;              /* whole icpmi_align* calls, device time */
    double loop_ms;                                  /* iteration loop + post-loop pass only */
    double setup_ms;                                 /* Morton sort + operand packing of the target */
    double nn_pairs;                                 /* (source,target) pairs evaluated by nn passes */
    int64_t nn_recheck_queries;                      /* extra 128-target slots scanned in fp64 (MFMA engine) */
    int64_t nn_fallback_queries;                     /* whole 2048-target splits re-scanned in fp64 */
    int64_t knn_fallback_rows;                       /* normal-estimation rows resolved by the exact k-NN kernel */
    int64_t nn_coarse_blocks;                        /* (512-query block, 2048-target split) workgroups launched */
    int64_t nn_pruned_blocks;                        /* of those, skipped by ICPMI_SEARCH_MFMA_PRUNED's box test */
    int64_t small_launches;                          /* iterations run by the small-cloud kernel (search + residuals + pose update in one launch) */
    int64_t bounded_launches;                        /* passes of the ICP loop searched behind a bound per row (lists instead of coarse minima) */
    int64_t nn_group_pairs;                          /* culled engine: (32-row tile, 2048-target split) pairs of its passes ... */
    int64_t nn_group_pairs_run;                      /* ... and those within reach, the ones the coarse pass evaluated */
    double exchange_ms;  int64_t exchange_launches;  /* sharded runs: the per-pass all-reduce of 30 doubles alone (the launches bracketed) */
    int64_t coarse_minima_bytes;                     /* bytes this context holds for (row, split) coarse minima (6 B each): only the
                                                        stand-alone nearest-neighbour search and ICPMI_NN_BOUNDED=0 reserve any -- no
                                                        registration does (a state, not a counter: icpmi_reset_profile leaves it) */
    int64_t nn_rows_listed;                          /* all-pairs engine with list reuse (ICPMI_NN_REUSE, default on): rows its bounded
                                                        passes listed again -- the others kept their lists -- and ... */
    int64_t nn_coarse_skipped;                       /* ... those passes whose coarse launch had no row to list, every workgroup left at
                                                        once.  With list reuse nn_pairs counts the pairs of the listed rows' workgroups;
                                                        both are counted on the device with profiling on only */
    int64_t knn_culled_launches;                     /* k-NN setup of a target (normal estimation): coarse passes run over the (32-row
                                                        group, split) pairs that survive the box test instead of all pairs -- both MFMA
                                                        engines on targets of more than 12 splits, engine 3 at every size */
    int64_t nn_rows_certified;                       /* all-pairs engine, match margin (ICPMI_NN_MARGIN, default on; sources of more
                                                        than 32,768 rows): rows of its bounded passes whose kept match was certified as
                                                        the unique nearest target -- neither listed nor scanned.  Profiling on only */
    int64_t nn_lean_passes;                          /* all-pairs engine, lean passes (ICPMI_NN_LEAN, default on; single-GPU ungated
                                                        loops over sources of 65,473 rows and more): passes queued without the row-list
                                                        and coarse launches, because the two latest passes the host knew of had
                                                        listed no row.  Counted on the host, profiling on or off */
    int64_t nn_full_culled_passes;                   /* all-pairs engine, culled full passes (ICPMI_NN_CULL_FULL, default on; single-GPU
                                                        ungated loops with list reuse and sorted rows -- sources of 4,096 rows and more -- over targets of 13 to 3,072 splits): the passes
                                                        that list every row -- a call's first two -- whose coarse launch ran over the
                                                        (32-row tile, split) pairs that survive the box test instead of all pairs.
                                                        Counted on the host, profiling on or off */
    int64_t nn_solo_passes;                          /* all-pairs engine, solo passes (ICPMI_NN_SOLO, default on; where lean passes and
                                                        the match margin are on, sources of 65,473 to 131,072 rows, profile < 2):
                                                        passes whose closing kernel also formed the next pass's terms and group sums,
                                                        because the two latest passes the host knew of had found every row certified;
                                                        that next pass launches its closing kernel only.  Counted on the host,
                                                        profiling on or off */
    int64_t nn_solo_fallback_rows;                   /* ... rows those kernels had to search themselves (exhaustively; profiling on) */
} icpmi_profile;

void icpmi_options_default(icpmi_options *opt);     /* device 0, normal_k 20 (icp.hpp:170), search AUTO or the
                                                        value of the environment variable ICPMI_SEARCH (0..3) */
void icpmi_config_default(icpmi_config *cfg);        /* types.hpp:143-148 defaults */

int icpmi_create(const icpmi_options *opt, icpmi_ctx **out);
void icpmi_destroy(icpmi_ctx *ctx);
const char *icpmi_last_error(const icpmi_ctx *ctx);  /* ctx may be NULL: last create error */
const char *icpmi_version(void);

/* Replaces slam::icp_point_to_plane (icp.hpp:157-258).  Host pointers.
 * error_history must hold max_iterations + 1 doubles (history_cap states its size). */
int icpmi_align(icpmi_ctx *ctx, const double *source_xyz, int64_t n_src,
                const double *target_xyz, int64_t n_tgt, const icpmi_config *cfg,
                icpmi_result *result, double *error_history, int32_t history_cap);

/* Same, with source/target already resident in this device's HBM (device pointers). */
int icpmi_align_device(icpmi_ctx *ctx, const double *d_source_xyz, int64_t n_src,
                       const double *d_target_xyz, int64_t n_tgt, const icpmi_config *cfg,
                       icpmi_result *result, double *error_history, int32_t history_cap);

/* Several independent registrations at once: the up-to-three ICP verifications of one
 * LoopClosureDetector::detect() (loop_closure.hpp:94-123), each a slam::icp_point_to_plane call of its own in
 * the reference.  Problem k runs on a stream and workspace of its own (helper contexts the library keeps
 * inside `ctx`, created on first use with ctx's options), driven by a host thread of its own, so the
 * registrations share the GPU: a filtered scan fills the chip for a part of each iteration only.
 * Every result is bit-identical to the same icpmi_align call made alone.  Host pointers; cfgs, results,
 * status: `count` entries; error_history: `count` rows of history_stride doubles (>= cfgs[k].max_iterations + 1).
 * status[k] is problem k's return code; the call returns ICPMI_OK if all are, else the first that is not
 * (its text in icpmi_last_error(ctx)).  1 <= count <= ICPMI_MAX_BATCH; not for a context with a communicator. */
#define ICPMI_MAX_BATCH 8
int icpmi_align_batch(icpmi_ctx *ctx, int32_t count, const double *const *sources_xyz, const int64_t *n_src,
                      const double *const *targets_xyz, const int64_t *n_tgt, const icpmi_config *cfgs,
                      icpmi_result *results, double *error_history, int32_t history_stride, int32_t *status);

/* The same registrations behind a correspondence-distance gate (not in the reference, which sums every source row into
 * the normal equations: icp.hpp:89-144).  With g2 = max_distance * max_distance a pass keeps row i, whose nearest target
 * is j, iff  e = q_j - p_i,  (e0 * e0 + e1 * e1) + e2 * e2 <= g2  in unfused fp64; a row with a non-finite coordinate is
 * dropped.  The sums run over the kept rows and the error is their RMS, sqrt(sum b^2 / kept); everything else -- the tests
 * in front of the solve, total = delta * total, the post-loop entry -- is icpmi_align's.  A pass that keeps no row ends
 * the call like a break without convergence: converged = 0, +Inf entered as that pass's error and again as the
 * post-loop entry, final_error = +Inf, the transform what had accumulated.  A gate that keeps every row gives
 * icpmi_align's bits.  max_distance must be finite and > 0 (ICPMI_ERR_ARG); "no gate" is icpmi_align*.  A context with
 * a communicator is refused (ICPMI_ERR_ARG).  Targets of up to 8 splits of 2,048 points run in the small-cloud kernel
 * as ungated ones do; beyond that every pass is a stand-alone search followed by the gated sums -- with the MFMA engines
 * that search keeps rows x splits x 6 B of coarse minima -- and is slower than the ungated loop.  A tight gate can make
 * the kept set alternate between passes, so that `tolerance` is never met; 2 m suits 0.5 m voxel-filtered street scans.
 * gate must not be NULL (ICPMI_ERR_NULL: "no gate" is icpmi_align*); its reserved[] is ignored.
 * info (may be NULL): pairs = rows kept by the pass that produced final_error, rows = n_src. */
typedef struct {
    double max_distance;           /* metres; finite, > 0 */
    int32_t reserved[2];
} icpmi_gate;
typedef struct {
    int64_t pairs;
    int64_t rows;
} icpmi_gate_info;
int icpmi_align_gated(icpmi_ctx *ctx, const double *source_xyz, int64_t n_src, const double *target_xyz, int64_t n_tgt,
                      const icpmi_config *cfg, const icpmi_gate *gate, icpmi_result *result, icpmi_gate_info *info,
                      double *error_history, int32_t history_cap);
int icpmi_align_gated_device(icpmi_ctx *ctx, const double *d_source_xyz, int64_t n_src, const double *d_target_xyz,
                             int64_t n_tgt, const icpmi_config *cfg, const icpmi_gate *gate, icpmi_result *result,
                             icpmi_gate_info *info, double *error_history, int32_t history_cap);
/* icpmi_align_batch with a gate per problem (gates: `count` entries; infos: `count` entries or NULL): every result is
 * bit-identical to the same icpmi_align_gated call made alone. */
int icpmi_align_gated_batch(icpmi_ctx *ctx, int32_t count, const double *const *sources_xyz, const int64_t *n_src,
                            const double *const *targets_xyz, const int64_t *n_tgt, const icpmi_config *cfgs,
                            const icpmi_gate *gates, icpmi_result *results, icpmi_gate_info *infos, double *error_history,
                            int32_t history_stride, int32_t *status);

/* The same registrations under robust row weights (not in the reference, which gives every source row the same say in
 * the normal equations: icp.hpp:89-144), optionally behind the correspondence-distance gate above.  Per pass, for row i
 * with nearest target j, in unfused fp64 and in this order:
 *     e  = q_j - p_i
 *     d2 = (e0*e0 + e1*e1) + e2*e2
 *     b  = (e0*n0 + e1*n1) + e2*n2          (icp.hpp:116)
 * Gate: the row is kept iff it has a neighbour and d2 <= g2, with g2 = max_distance*max_distance when a gate is given
 * and g2 = DBL_MAX when max_distance == 0; a NaN or infinite row is then still dropped.
 * Weight of a kept row, a = fabs(b), k = scale:
 *     ICPMI_ROBUST_HUBER           w = a <= k ? 1.0 : k / a
 *     ICPMI_ROBUST_GEMAN_MCCLURE   s = k*k (formed on the host, once), t = s + b*b, r = s / t, w = r*r
 * Sums over the kept rows, wJ[r] = w*J[r]: the 21 JtJ sums add wJ[r]*J[c], the 6 Jtb sums add wJ[r]*b, the squared
 * error adds (w*b)*b, the weight sum adds w and the pairs add 1.0; a dropped row adds nothing.  With w == 1.0 every
 * product is the unweighted one: a Huber scale above every |b| gives icpmi_align_gated's bits, and with no gate
 * icpmi_align's.
 * Error: sqrt(sum w b^2 / sum w), the WEIGHTED RMS; it is final_error, the history and what both stopping tests read,
 * and it reads lower than the plain RMS of the same pose -- a caller's thresholds on final_error (the reference node's
 * `> 1.0`, a loop detector's fitness `< 0.3`, a pose graph's odometry noise) see that number.
 * A pass whose weight sum is not > 0 ends the call as a gated pass that keeps no row does (icpmi_align_gated).  The step,
 * total = delta * total, the post-loop entry and the history invariants are icpmi_align's.
 * A redescending weight needs a start inside its basin: Geman-McClure at a scale far below the start's residuals locks
 * onto the start (0.1 m with a start a metre off stays a metre off); Huber does not redescend.
 * Validation: scale finite and > 0; kind one of the two; max_distance 0 or finite and > 0 -- anything else is
 * ICPMI_ERR_ARG; a NULL rule is ICPMI_ERR_NULL; a context with a communicator is refused (ICPMI_ERR_ARG).  Paths as
 * icpmi_align_gated's: the small-cloud kernel in the small regime, else a stand-alone search plus the weighted sums.
 * info (may be NULL): weight_sum and pairs of the pass that produced final_error, rows = n_src. */
#define ICPMI_ROBUST_HUBER 1
#define ICPMI_ROBUST_GEMAN_MCCLURE 2
typedef struct {
    int32_t kind;                  /* ICPMI_ROBUST_* */
    int32_t reserved;
    double scale;                  /* k, in metres of point-to-plane residual; finite, > 0 */
    double max_distance;           /* the gate, metres; 0: none */
} icpmi_robust;
typedef struct {
    double weight_sum;
    int64_t pairs;
    int64_t rows;
} icpmi_robust_info;
int icpmi_align_robust(icpmi_ctx *ctx, const double *source_xyz, int64_t n_src, const double *target_xyz, int64_t n_tgt,
                       const icpmi_config *cfg, const icpmi_robust *rule, icpmi_result *result, icpmi_robust_info *info,
                       double *error_history, int32_t history_cap);
int icpmi_align_robust_device(icpmi_ctx *ctx, const double *d_source_xyz, int64_t n_src, const double *d_target_xyz,
                              int64_t n_tgt, const icpmi_config *cfg, const icpmi_robust *rule, icpmi_result *result,
                              icpmi_robust_info *info, double *error_history, int32_t history_cap);
/* icpmi_align_batch with a rule per problem (rules: `count` entries; infos: `count` entries or NULL): every result is
 * bit-identical to the same icpmi_align_robust call made alone. */
int icpmi_align_robust_batch(icpmi_ctx *ctx, int32_t count, const double *const *sources_xyz, const int64_t *n_src,
                             const double *const *targets_xyz, const int64_t *n_tgt, const icpmi_config *cfgs,
                             const icpmi_robust *rules, icpmi_result *results, icpmi_robust_info *infos,
                             double *error_history, int32_t history_stride, int32_t *status);

/* Plane-to-plane (generalized) ICP: the same registrations with a local surface model on BOTH clouds (Segal's
 * Generalized-ICP; not in the reference, whose cost is point-to-plane: icp.hpp:89-144), optionally behind the
 * correspondence-distance gate above.  The plane-regularised covariance U diag(1, 1, epsilon) U^T of a row with unit
 * normal n is I - (1 - epsilon) n n^T, so the normals are all either side needs and no eigendecomposition is run.
 *
 * Per pass, for row i of the moved source `cur` with nearest target j (`found`: the row has a neighbour), in unfused
 * fp64 and in this order:
 *     R    = rotation block of IcpState::total as the pass finds it (total[0..2], [4..6], [8..10])
 *     s    = normal of source row i, estimated ONCE per call on the source as the caller gave it
 *            (before initial_transform; k = options.normal_k; the normals launch_normals gives)
 *     m_a  = (R[a][0]*s0 + R[a][1]*s1) + R[a][2]*s2
 *     n    = normal of target j;  p = cur_i;  e = q_j - p;  d2 = (e0*e0 + e1*e1) + e2*e2
 *     kept iff found && d2 <= g2      (g2 = max_distance^2, or DBL_MAX when max_distance == 0)
 *     c = 1 - epsilon, kappa = 2*epsilon            (formed once on the host)
 *     S_ab = (a==b ? 2.0 : 0.0) - c*(n_a*n_b + m_a*m_b)          for a <= b
 *     C00 = S11*S22 - S12*S12;  C01 = S02*S12 - S01*S22;  C02 = S01*S12 - S02*S11
 *     C11 = S00*S22 - S02*S02;  C12 = S01*S02 - S00*S12;  C22 = S00*S11 - S01*S01
 *     det = (S00*C00 + S01*C01) + S02*C02;  r = 1.0/det;  M_ab = C_ab*r      (one division per kept row)
 *     u_a = (M_a0*e0 + M_a1*e1) + M_a2*e2
 *     A   = [ -[p]x | I ]:  A0 = (0, p2, -p1, 1,0,0), A1 = (-p2, 0, p0, 0,1,0), A2 = (p1, -p0, 0, 0,0,1)
 *     B   = [p]x M (rows 0..2 against columns 3..5 of A^T M A; M_ab = M_ba):
 *           B0c = p1*M2c - p2*M1c;  B1c = p2*M0c - p0*M2c;  B2c = p0*M1c - p1*M0c
 *     G   = B (-[p]x) (rows and columns 0..2), for r <= c only:
 *           Gr0 = Br2*p1 - Br1*p2;  Gr1 = Br0*p2 - Br2*p0;  Gr2 = Br1*p0 - Br0*p1
 *     v   = p x u:  v0 = p1*u2 - p2*u1;  v1 = p2*u0 - p0*u2;  v2 = p0*u1 - p1*u0
 * Columns of a kept row (the gated call's layout; a dropped row adds nothing):
 *     0..20   the upper triangle of A^T M A, row by row:
 *             G00 G01 G02 B00 B01 B02 | G11 G12 B10 B11 B12 | G22 B20 B21 B22 | M00 M01 M02 | M11 M12 | M22
 *     21..26  A^T u = v0 v1 v2 u0 u1 u2
 *     27      kappa * ((e0*u0 + e1*u1) + e2*u2)
 *     28      1.0
 * The step solves H x = g with H = sum A^T M A and g = sum A^T M e, as icpmi_align's solves JtJ x = Jtb (in the
 * point-to-plane limit M = n n^T they are the same sums); icpmi_last_normal_matrix hands them over as JtJ, Jtb, sum_sq
 * and weight = pairs.
 * Error: final_error, the history and what both stopping tests read is sqrt(sum kappa e^T M e / pairs).  The factor
 * kappa = 2 epsilon makes it read in METRES: with parallel normals kappa e^T M e = (e.n)^2 + epsilon * (tangential)^2, the
 * point-to-plane residual plus a small tangential term.  Without it the Mahalanobis RMS would be 1/sqrt(2 epsilon) times
 * larger and a caller's thresholds on final_error (the reference node's `> 1.0`, a loop detector's fitness `< 0.3`,
 * `tolerance`, `min_error`) would all mean something else.
 * epsilon = 1 gives S = 2 I and M = I / 2 exactly: point-to-point ICP.
 * A pass that keeps no row ends the call as icpmi_align_gated's does; the step, total = delta * total, the post-loop
 * entry and the history invariants are icpmi_align's.  A non-finite source row is dropped by the d2 test.
 * Validation: epsilon finite with 0 < epsilon <= 1; max_distance 0 or finite and > 0 -- anything else is ICPMI_ERR_ARG; a
 * NULL rule is ICPMI_ERR_NULL; a context with a communicator is refused (ICPMI_ERR_ARG).
 * Path: at every size a stand-alone search on the context's engine, then the plane-to-plane sums, the gated step and the
 * rows' move; the source's normals cost one 20-NN pass over the source per call, in front of the target's preparation,
 * and a target the context had remembered is forgotten by such a call.
 * Form (bit 0 of `reserved`, ICPMI_GICP_FORM_SMALL; the other bits are ignored): with it, a call whose sizes the small-cloud
 * kernel takes -- a source of at most 32,768 rows, a target within its 8 splits of 2,048 points on the bf16 MFMA engine, no
 * communicator -- runs each pass's search, rows and sums in ONE kernel, as icpmi_align_gated does at those sizes; at other
 * sizes the bit has no effect.  The rows are the ones above, word for word; they are ADDED in the small-cloud kernel's
 * order, not the general path's, so the two forms agree to rounding, not to bits.  0 is the general path at every size.
 * info (may be NULL): pairs = rows kept by the pass that produced final_error, rows = n_src. */
#define ICPMI_GICP_EPSILON_DEFAULT 1e-3
#define ICPMI_GICP_FORM_SMALL 1
typedef struct {
    double epsilon;                /* the covariance along the normal, relative to 1 in the plane; finite, 0 < epsilon <= 1 */
    double max_distance;           /* the gate, metres; 0: none */
    int64_t reserved;              /* bit 0: ICPMI_GICP_FORM_SMALL; 0: the general path */
} icpmi_gicp;
typedef struct {
    int64_t pairs;
    int64_t rows;
} icpmi_gicp_info;
int icpmi_align_gicp(icpmi_ctx *ctx, const double *source_xyz, int64_t n_src, const double *target_xyz, int64_t n_tgt,
                     const icpmi_config *cfg, const icpmi_gicp *rule, icpmi_result *result, icpmi_gicp_info *info,
                     double *error_history, int32_t history_cap);
int icpmi_align_gicp_device(icpmi_ctx *ctx, const double *d_source_xyz, int64_t n_src, const double *d_target_xyz,
                            int64_t n_tgt, const icpmi_config *cfg, const icpmi_gicp *rule, icpmi_result *result,
                            icpmi_gicp_info *info, double *error_history, int32_t history_cap);
/* icpmi_align_batch with a rule per problem (rules: `count` entries, each with its own form; infos: `count` entries or
 * NULL): every result is bit-identical to the same icpmi_align_gicp call made alone. */
int icpmi_align_gicp_batch(icpmi_ctx *ctx, int32_t count, const double *const *sources_xyz, const int64_t *n_src,
                           const double *const *targets_xyz, const int64_t *n_tgt, const icpmi_config *cfgs,
                           const icpmi_gicp *rules, icpmi_result *results, icpmi_gicp_info *infos,
                           double *error_history, int32_t history_stride, int32_t *status);

/* The normal equations of the pass that produced final_error of the last registration this context ran: what the
 * registration minimised, at its result.  Costs nothing: the sums come back with the result behind the call's one wait,
 * and this getter only copies them on the host.
 *   JtJ     row-major 6 x 6, symmetric: sum w J^T J over the pass's pairs, J = [(p x n)^T, n^T], p the source point moved by
 *           T, n the normal of its nearest target point, in the order [rotation; translation] of the registration's step
 *           (a left perturbation of T in the target frame).  Filled from the 21 sums of the upper triangle, bits copied.
 *   Jtb     sum w J^T b, b = (q - p) . n with q the matched target point: the step solves JtJ x = Jtb
 *   sum_sq  sum w b^2;  final_error = sqrt(sum_sq / weight), to the bit
 *   weight  the divisor: the pairs of a plain or gated call, the weight sum of a robust one (w is 1 except there)
 *   pairs   rows that entered the sums
 *   T       the registration's result
 * After a loop that broke on a convergence test these are the breaking pass's sums, after an exhausted loop the
 * post-loop pass's; either way the pass ran at T.  k: the problem of the last icpmi_align*_batch call, 0 after a single
 * call (host or device entry, plain, gated, robust or plane-to-plane, icpmi_stream_push*, icpmi_local_map_register*).
 * ICPMI_ERR_ARG, with a text in icpmi_last_error: k out of range; no registration ran (a fresh context, a stream push
 * that registered nothing, a call that failed); a gated or robust pass that kept no row; a context with a
 * communicator (its sums are the ranks' shares). */
typedef struct {
    double JtJ[36];
    double Jtb[6];
    double sum_sq;
    double weight;
    int64_t pairs;
    double T[16];
} icpmi_normal_matrix;
int icpmi_last_normal_matrix(icpmi_ctx *ctx, int32_t k, icpmi_normal_matrix *out);

/* Replaces KDTree(points) + KDTree::nearest_batch (kdtree.hpp:20-26,43-59): for each
 * query the index of, and squared distance to, its nearest target.  Host pointers;
 * dist_sq may be NULL. */
int icpmi_nearest_batch(icpmi_ctx *ctx, const double *targets_xyz, int64_t n_tgt,
                        const double *queries_xyz, int64_t n_qry, int32_t *indices,
                        double *dist_sq);

/* Replaces KDTree::k_nearest (kdtree.hpp:65-78) for a batch of query points: indices (n_qry x k,
 * row-major) of the k nearest targets of every query, closest first as kdtree.hpp:72-76 returns
 * them; equal distances in ascending index order.  A target used as a query finds itself
 * first (distance 0), like the reference.  1 <= k <= 64.  Entries a list does not reach
 * (k > n_tgt; a query with a NaN coordinate) are -1 with distance +infinity.  dist_sq (n_qry x
 * k) may be NULL.  Host pointers. */
int icpmi_k_nearest(icpmi_ctx *ctx, const double *targets_xyz, int64_t n_tgt,
                    const double *queries_xyz, int64_t n_qry, int32_t k, int32_t *indices,
                    double *dist_sq);

/* Replaces estimate_normals(points, tree, k) (icp.hpp:23-67).  Host pointers. */
int icpmi_estimate_normals(icpmi_ctx *ctx, const double *points_xyz, int64_t n, int32_t k,
                           double *normals_xyz);

/* Replaces solve_point_to_plane(source, target, normals) (icp.hpp:89-144): inputs are
 * three n x 3 arrays matched row by row; out is the row-major 4x4 update. */
int icpmi_solve_point_to_plane(icpmi_ctx *ctx, const double *source_xyz,
                               const double *target_xyz, const double *normals_xyz, int64_t n,
                               double transform_out[16]);

/* Replaces Transformation::apply(cloud) (types.hpp:110-115): out = in * R^T + t^T. */
int icpmi_transform_points(icpmi_ctx *ctx, const double transform[16], const double *in_xyz,
                           int64_t n, double *out_xyz);

/* Replaces voxel_downsample(points, voxel_size) (slam_viz/src/core/file_utils.cpp:148-196), the
 * step slam_node.cpp:122 runs before every registration: centroid of the points of each
 * occupied voxel, key = floor(coord / voxel_size), points summed in input order.  Voxels come
 * out sorted by key (the reference's order is std::unordered_map iteration order, i.e.
 * implementation-defined).  voxel_size <= 0 copies the input (file_utils.cpp:152).  out_cap
 * is in rows; n rows always suffice.  The grid may span at most 2^21 cells per axis; a point with a NaN or
 * infinite coordinate (undefined behaviour in the reference: the cast of floor(NaN)) is ICPMI_ERR_ARG. */
int icpmi_voxel_downsample(icpmi_ctx *ctx, const double *points_xyz, int64_t n, double voxel_size,
                           double *out_xyz, int64_t out_cap, int64_t *n_out);
/* Same on device pointers (the result can feed icpmi_align_device without leaving HBM). */
int icpmi_voxel_downsample_device(icpmi_ctx *ctx, const double *d_points_xyz, int64_t n,
                                  double voxel_size, double *d_out_xyz, int64_t out_cap,
                                  int64_t *n_out);

/* Replaces load_ply / load_bin (slam_viz/src/core/file_utils.cpp:20-108, 115-141; the node
 * calls load_ply at slam_node.cpp:69,121): a path ending in ".bin" is read as KITTI
 * (x, y, z, intensity float32, intensity dropped), anything else as PLY with the reference's
 * header rules.  Host-side only (no context, no device).  Two-call pattern: with out_xyz ==
 * NULL only *n_out is set.  A file that cannot be opened returns ICPMI_ERR_ARG (the
 * reference throws std::runtime_error). */
int icpmi_load_cloud(const char *path, double *out_xyz, int64_t cap, int64_t *n_out);
/* Replaces discover_frames + extract_timestamp (slam_viz/src/core/file_utils.cpp:203-247): the
 * entries of data_dir whose extension is ".ply" or ".bin" and whose name holds a run of digits in
 * front of that extension, sorted by that number (equal numbers by path).  Two-call pattern: with
 * stamps == paths == NULL only *n_frames and *paths_bytes are set; then stamps[n_frames] and
 * paths (NUL-terminated strings, one after the other, paths_bytes in all) are filled.  A
 * directory that cannot be opened returns ICPMI_ERR_ARG (the reference throws).  Host-side. */
int icpmi_discover_frames(const char *data_dir, int64_t *stamps, int64_t frames_cap, char *paths,
                          int64_t paths_cap, int64_t *n_frames, int64_t *paths_bytes);

/* The device form of load_bin (file_utils.cpp:115-141): host float32 records (x, y, z leading,
 * stride_floats apart: 4 for KITTI) are copied to the device as they are and widened to the
 * N x 3 fp64 layout there (static_cast<double> is exact either side): 16 instead of 24 bytes per
 * point cross the host link.  d_out_xyz: device pointer, n rows. */
int icpmi_upload_points_f32(icpmi_ctx *ctx, const float *records, int64_t n, int32_t stride_floats,
                            double *d_out_xyz);
/* icpmi_load_cloud into device memory: ".bin" through icpmi_upload_points_f32, PLY parsed on the
 * host (header rules, ASCII numbers) and uploaded as fp64.  Two-call pattern like icpmi_load_cloud
 * (d_out_xyz == NULL: only *n_out). */
int icpmi_load_cloud_device(icpmi_ctx *ctx, const char *path, double *d_out_xyz, int64_t cap,
                            int64_t *n_out);

/* estimate_normals (icp.hpp:23-67) for rows [row0, row1) of the cloud only, against the whole
 * cloud: what one rank of a job that shards the normal estimation itself computes.  normals_xyz
 * receives row1 - row0 rows.  Host pointers. */
int icpmi_estimate_normals_rows(icpmi_ctx *ctx, const double *points_xyz, int64_t n, int32_t k,
                                int64_t row0, int64_t row1, double *normals_xyz);

/* One step of frame-to-frame odometry with the clouds resident in HBM: the registration part of
 * SlamNode::process_frame (slam_viz/src/ros/slam_node.cpp:122-152).
 *     curr = voxel_downsample(raw, voxel_size)                       :122
 *     first frame: keep it, nothing to register                      :69-72   -> ICPMI_STREAM_FIRST_FRAME
 *     curr.rows() < min_points: keep it, caller repeats its last pose :125-130 -> ICPMI_STREAM_TOO_FEW_POINTS
 *     result = icp_point_to_plane(source = curr, target = prev, cfg) :132-138 -> ICPMI_STREAM_REGISTERED
 *     prev = curr                                                    :128,152
 * The context keeps the previous filtered scan in device memory (the target of frame t+1 is the
 * source of frame t; buffers are swapped, nothing is copied or uploaded twice), builds the
 * target's search structure and normals from that resident copy, and the caller applies the
 * reference's gate (!converged || final_error > 1.0 -> identity, :139-140) and pose update.
 * d_raw_xyz: device pointer to the raw scan (e.g. from icpmi_load_cloud_device).  In the first
 * two cases *result is the identity with converged = 0 and no history. */
#define ICPMI_STREAM_REGISTERED 0
#define ICPMI_STREAM_FIRST_FRAME 1
#define ICPMI_STREAM_TOO_FEW_POINTS 2
typedef struct {
    int32_t status;      /* ICPMI_STREAM_* */
    int32_t reserved;
    int64_t n_filtered;  /* rows of the filtered current scan (now the resident "previous" one) */
    int64_t n_target;    /* rows of the scan it was registered against */
} icpmi_stream_info;
int icpmi_stream_push(icpmi_ctx *ctx, const double *d_raw_xyz, int64_t n_raw, double voxel_size,
                      int64_t min_points, const icpmi_config *cfg, icpmi_result *result,
                      double *error_history, int32_t history_cap, icpmi_stream_info *info);
/* Same with the raw scan in host memory (uploaded once; the filtered scan still never leaves the device). */
int icpmi_stream_push_host(icpmi_ctx *ctx, const double *raw_xyz, int64_t n_raw, double voxel_size,
                           int64_t min_points, const icpmi_config *cfg, icpmi_result *result,
                           double *error_history, int32_t history_cap, icpmi_stream_info *info);
/* Same with the raw scan in a file (load_ply / load_bin, file_utils.cpp:20-141, what slam_node.cpp:121
 * reads): a KITTI ".bin" goes from disk through pinned memory to the device as float32 and
 * everything behind the read is queued without a wait in between; a PLY takes the host parser. */
int icpmi_stream_push_file(icpmi_ctx *ctx, const char *path, double voxel_size, int64_t min_points,
                           const icpmi_config *cfg, icpmi_result *result, double *error_history,
                           int32_t history_cap, icpmi_stream_info *info);
/* Start bringing the NEXT frame file to the device on a worker thread of the context and return at once:
 * the file is read into pinned memory (~140 us for a 1.8 MB scan out of the page cache), copied over on a
 * stream of the worker's own, widened and -- with the voxel size of the stream's last push -- filtered there;
 * the icpmi_stream_push_file of that same path then starts at the registration (it waits for the worker if it
 * is still busy with that file; with another voxel size it filters the raw points, already on the device, itself).  Call it BEFORE
 * pushing the current frame: read and copy then run beside the current frame's work.  KITTI ".bin" only (a
 * PLY is parsed when pushed: the call is a no-op); one file at a time; a finished file is kept until the
 * push of its path takes it (at most two wait, the older gives way to a third); a file that cannot be read
 * is reported by the push.  Never needed for correctness. */
int icpmi_stream_prefetch_file(icpmi_ctx *ctx, const char *path);
int icpmi_stream_reset(icpmi_ctx *ctx);   /* forget the resident frame (a new sequence starts) */
/* Robust row weights for the stream (icpmi_align_robust's rule and validation; NULL: off, as at creation): every later
 * icpmi_stream_push* registers under the rule, bit-identical to icpmi_align_robust on the same filtered scans.  The next
 * target's early preparation on the helper context, and its adoption, are untouched.  The rule survives
 * icpmi_stream_reset.  icpmi_stream_last_robust: weight_sum, pairs and rows of the last push's registration; all zero
 * when that push registered nothing or ran without a rule. */
int icpmi_stream_set_robust(icpmi_ctx *ctx, const icpmi_robust *rule);
int icpmi_stream_last_robust(icpmi_ctx *ctx, icpmi_robust_info *info);

/* The map side of SlamNode::process_frame, once the caller has formed new_pose = poses.back() * delta
 * (slam_viz/src/ros/slam_node.cpp:142-153):
 *     world = curr * new_pose.R^T + new_pose.t^T                    :147
 *     update_occupancy_grid(world, new_pose.t)                      :153, :211-221
 * update_occupancy_grid marks, for every world point with height_min <= z <= height_max and
 * 0.5 <= hypot(x - sensor.x, y - sensor.y) <= max_range, the 2-D cell (floor(x / resolution),
 * floor(y / resolution)) in a set of cells (std::unordered_set<GridCell>, slam_node.hpp:45-58); the
 * defaults are OccupancyGridConfig's (slam_node.hpp:35-40).  Here the set lives in device memory
 * as a sorted array of unique cells that every update merges into.  Beyond the reference: a point
 * whose quotient is not finite or does not fit an int (undefined static_cast there) marks nothing. */
typedef struct {
    double resolution;   /* 0.2 */
    double height_min;   /* 0.3 */
    double height_max;   /* 2.0 */
    double max_range;    /* 40.0 */
} icpmi_grid_config;
void icpmi_grid_config_default(icpmi_grid_config *grid);
/* world points in host memory (n x 3) and the sensor position; *n_cells (may be NULL: no wait for
 * the device then) receives the size of the set after the update. */
int icpmi_occupancy_update(icpmi_ctx *ctx, const double *world_xyz, int64_t n, const double sensor_xyz[3],
                           const icpmi_grid_config *grid, int64_t *n_cells);
/* Same with the points in device memory. */
int icpmi_occupancy_update_device(icpmi_ctx *ctx, const double *d_world_xyz, int64_t n, const double sensor_xyz[3],
                                  const icpmi_grid_config *grid, int64_t *n_cells);
/* The set: cells_xy[2 i], cells_xy[2 i + 1] = (x, y) of cell i, sorted by x then y.  cells_xy may be
 * NULL (only *n_cells is set); fewer than *n_cells entries of capacity is ICPMI_ERR_CAPACITY.  What
 * cells_to_occupancy_grid_msg (slam_node.cpp:279-297) rasterises. */
int icpmi_occupancy_cells(icpmi_ctx *ctx, int32_t *cells_xy, int64_t cap_cells, int64_t *n_cells);
int icpmi_occupancy_clear(icpmi_ctx *ctx);   /* occupied_cells_.clear() (slam_node.cpp:224) */
/* The filtered scan the last icpmi_stream_push* left resident (`curr`, slam_node.cpp:122), copied to the host:
 * what the node hands to loop_detector_.addFrame and keeps in downsampled_clouds_ (:160).  out_xyz may be
 * NULL (only *n_out is set).  The stream itself never needs this copy. */
int icpmi_stream_current_scan(icpmi_ctx *ctx, double *out_xyz, int64_t cap, int64_t *n_out);
/* Both steps on the scan the last icpmi_stream_push* left resident (it never came to the host):
 * pose = new_pose, row-major 4 x 4.  world_out (host, may be NULL) receives the n_filtered x 3 world
 * points (what publish_current_scan sends, :155), *n_world their number; grid may be NULL (no grid
 * update; *n_cells is then the current size).  One wait for everything the call returns. */
int icpmi_stream_map_update(icpmi_ctx *ctx, const double pose[16], const icpmi_grid_config *grid,
                            double *world_out, int64_t world_cap, int64_t *n_world, int64_t *n_cells);

/* Replaces ScanContext::compute (core/scan_context.hpp:44-82): 20 rings x 60 sectors max-height
 * descriptor, row-major desc_out[ring * 60 + sector], empty bins 0. */
#define ICPMI_SC_RINGS 20
#define ICPMI_SC_SECTORS 60
int icpmi_scan_context(icpmi_ctx *ctx, const double *cloud_xyz, int64_t n, double *desc_out /* 1200 */);
/* Replaces the loop of ScanContext::distance calls in LoopClosureDetector::detect
 * (core/loop_closure.hpp:78-89, core/scan_context.hpp:90-142): dist_out[i] = min over the 60
 * column shifts of 1 - cosine(query, hist_descs + 1200 * i). */
int icpmi_scan_context_distances(icpmi_ctx *ctx, const double *query_desc, const double *hist_descs,
                                 int64_t count, double *dist_out);
/* The same call with the argmin kept (not in the reference, which drops it at scan_context.hpp:94-99): dist_out is
 * icpmi_scan_context_distances' bit for bit, shift_out[i] in 0..59 the SMALLEST column shift that attains dist_out[i]
 * (the reference's loop runs upward with a strict <).  query[ring][j] was compared with hist[ring][(j + shift) % 60],
 * so the shift is the yaw between the two scans to within half a sector.  Where a per-shift distance is NaN the shift
 * is some value in 0..59. */
int icpmi_scan_context_distances_shift(icpmi_ctx *ctx, const double *query_desc, const double *hist_descs,
                                       int64_t count, double *dist_out, int32_t *shift_out);
/* The initial transform a loop-closure verification takes from that shift, query = source, candidate = target:
 * row-major Rz(shift * (2.0 * M_PI / 60)) by the C library's cos and sin; shift 0 is the exact identity.  A shift
 * outside 0..59 is ICPMI_ERR_ARG.  Host only: no context, no device.  The one definition of the guess. */
int icpmi_sc_shift_transform(int32_t shift, double T[16]);

/* Multi-GPU (new; the reference has no distributed path).  One process per GPU.  Rank 0
 * obtains an id, the host distributes it (e.g. torch.distributed broadcast), every rank
 * calls icpmi_comm_init.  Afterwards icpmi_align* treats `source` as this rank's shard
 * of the source cloud; the target is replicated.  Each iteration all-reduces 30 doubles
 * (21 J^T J + 6 J^T b + sum b^2 + count + the number of ranks whose loop has ended) over RCCL.
 * Every rank must make the same calls with the same icpmi_config and target.  A shard may be
 * empty (n_src == 0, source pointer ignored) as long as some rank holds points: it adds
 * nothing to the sums and takes part in every exchange.  The ranks stop on the exchanged
 * count of finished loops, never on a local decision, so they always queue the same number
 * of collectives; if they did not all finish at the same iteration (configs differ, or an
 * exchange that is not bit-identical on every rank) every rank returns ICPMI_ERR_RCCL from
 * that call instead of waiting for the others forever. */
#define ICPMI_UNIQUE_ID_BYTES 128
int icpmi_comm_unique_id(icpmi_ctx *ctx, void *id_out /* ICPMI_UNIQUE_ID_BYTES */);
int icpmi_comm_init(icpmi_ctx *ctx, int32_t n_ranks, int32_t rank, const void *id);
int icpmi_comm_finalize(icpmi_ctx *ctx);

/* Same sharded path with the two exchanges done by host callbacks instead of RCCL (the
 * buffers are host memory; the callee must leave the result in place).  Meant for
 * rehearsing the N > 1 path where RCCL cannot run (several ranks on one GPU, gloo). */
typedef int (*icpmi_allreduce_fn)(void *user, double *buf, int32_t count);            /* in-place sum */
typedef int (*icpmi_allgather_fn)(void *user, double *buf, int32_t count_per_rank);   /* in-place, rank-major */
int icpmi_comm_init_callbacks(icpmi_ctx *ctx, int32_t n_ranks, int32_t rank,
                              icpmi_allreduce_fn allreduce, icpmi_allgather_fn allgather,
                              void *user);

/* Who is in this context's communicator, asked of the communicator itself (new, like the rest of the multi-GPU
 * section: no reference counterpart): n_ranks / rank / this rank's device from ncclCommCount / ncclCommUserRank /
 * ncclCommCuDevice, and every rank's device ordinal and PCI bus id gathered through the library's own all-gather --
 * so that a scaling line can prove how many distinct GPUs its ranks ran on.  A collective: every rank calls it.
 * kind: 0 no communicator (n_ranks 1), 1 RCCL, 2 host callbacks (n_ranks as given to icpmi_comm_init_callbacks). */
#define ICPMI_MAX_RANKS_INFO 64
typedef struct {
    int32_t kind, n_ranks, rank, reserved;
    int32_t device[ICPMI_MAX_RANKS_INFO];
    char pci_bus_id[ICPMI_MAX_RANKS_INFO][16];
} icpmi_comm_info_t;
int icpmi_comm_info(icpmi_ctx *ctx, icpmi_comm_info_t *out);

/* Pose graph: replaces slam::PoseGraph (core/pose_graph.hpp:49-147, src/core/pose_graph.cpp), the GTSAM
 * Levenberg-Marquardt back end the node feeds one odometry factor per frame (slam_node.cpp:145) and one factor per
 * accepted loop closure (:163), and re-optimises after a pending closure (:112-115) and at the end (:106).
 * Objective 0.5 sum ||r||^2_Sigma with GTSAM 4.x Pose3 (EXPMAP build), tangent order (omega, v); the LM policy is
 * GTSAM's defaults (lambda 1e-5, factor 10, upper bound 1e5, minModelFidelity 1e-3, H + lambda I).  The factors and
 * estimates live in device buffers owned by the handle; optimize() uploads what was added since the last call and
 * reads back two doubles per lambda trial.  A handle uses its context's device and stream: one caller thread at a
 * time, never overlapping the context's own calls.  Transforms are row-major double[16]; rotations are taken as given
 * (Rot3(Matrix3)), not re-orthonormalised.  A non-finite entry, or from == to, is ICPMI_ERR_ARG. */
typedef struct icpmi_pose_graph icpmi_pose_graph;
typedef struct {                     /* slam::PoseGraphConfig, pose_graph.hpp:22-40 */
    double odom_rotation_sigma;      /* 0.01 rad */
    double odom_translation_sigma;   /* 0.05 m */
    double prior_rotation_sigma;     /* 0.001 */
    double prior_translation_sigma;  /* 0.001 */
    double loop_rotation_sigma;      /* 0.005 */
    double loop_translation_sigma;   /* 0.025 */
    int32_t max_iterations;          /* 100 */
    int32_t reserved;
    double relative_error_tol;       /* 1e-5 */
    double absolute_error_tol;       /* 1e-5 */
} icpmi_pose_graph_config;

#define ICPMI_PG_STOP_NONE 0
#define ICPMI_PG_STOP_ZERO_ERROR 1        /* error <= errorTol (0) */
#define ICPMI_PG_STOP_MAX_ITERATIONS 2
#define ICPMI_PG_STOP_RELATIVE 3          /* checkConvergence: relative decrease <= relative_error_tol */
#define ICPMI_PG_STOP_ABSOLUTE 4          /* checkConvergence: absolute decrease <= absolute_error_tol */
#define ICPMI_PG_STOP_LAMBDA_BOUND 5      /* tryLambda: lambda reached 1e5 without a successful step */
#define ICPMI_PG_STOP_SMALL_COST_CHANGE 6 /* tryLambda: |cost change| < relative_error_tol * error, no step taken */
#define ICPMI_PG_STOP_NOT_FINITE 7

typedef struct {
    int32_t optimized;         /* 1: optimize() returned true (optimized_ set) */
    int32_t iterations;        /* LevenbergMarquardtOptimizer::iterations(): successful steps */
    int32_t inner_iterations;  /* lambda trials (tryLambda calls) */
    int32_t stop_reason;       /* ICPMI_PG_STOP_* */
    double initial_error;
    double final_error;        /* optimizer.error() (pose_graph.cpp:159) */
    double final_lambda;
    int32_t history_len;       /* initial error + one entry per outer iteration */
    int32_t reserved;
} icpmi_pose_graph_info;

void icpmi_pose_graph_config_default(icpmi_pose_graph_config *cfg);   /* pose_graph.hpp:25-39 */
/* PoseGraph::PoseGraph (pose_graph.cpp:10-16); cfg NULL: defaults */
int icpmi_pose_graph_create(icpmi_ctx *ctx, const icpmi_pose_graph_config *cfg, icpmi_pose_graph **out);
void icpmi_pose_graph_destroy(icpmi_pose_graph *graph);
/* addPrior (pose_graph.cpp:58-79): prior with sigmas (rotation, translation); inserts pose as the estimate of index
 * if it has none.  Does not clear the optimised state (the reference's quirk). */
int icpmi_pose_graph_add_prior(icpmi_pose_graph *graph, int64_t index, const double pose[16]);
/* addOdometryFactor (:81-116): sigmas scaled by 1 + 10 fitness; `to` gets X_from * rel if it has no estimate.  Where
 * the reference throws (no estimate for `from` either), ICPMI_ERR_ARG and the graph is unchanged. */
int icpmi_pose_graph_add_odometry(icpmi_pose_graph *graph, int64_t from, int64_t to, const double rel[16],
                                  double fitness);
/* addLoopClosure (:118-141): loop sigmas, counted, no estimate added */
int icpmi_pose_graph_add_loop_closure(icpmi_pose_graph *graph, int64_t from, int64_t to, const double rel[16]);
/* optimize (:147-171), always from the initial estimates.  Empty graph: ICPMI_OK with info->optimized 0 (the
 * reference returns false).  A factor on a pose with no estimate: ICPMI_ERR_ARG (the reference's catch returns
 * false), nothing changes.  info may be NULL; history (may be NULL) receives info->history_len errors and needs
 * max_iterations + 1 entries (else ICPMI_ERR_CAPACITY). */
int icpmi_pose_graph_optimize(icpmi_pose_graph *graph, icpmi_pose_graph_info *info, double *history,
                              int32_t history_cap);
/* getPose (:177-186): optimised values while optimized_ holds, initial estimates otherwise; a missing index is
 * ICPMI_ERR_ARG. */
int icpmi_pose_graph_pose(icpmi_pose_graph *graph, int64_t index, double pose[16]);
/* getAllPoses (:188-200): indices 0 .. size()-1 with an estimate, in order.  *n_out receives their number; poses
 * (count x 16) and indices (count; the pose index of each) may be NULL; fewer than *n_out of capacity is
 * ICPMI_ERR_CAPACITY. */
int icpmi_pose_graph_poses(icpmi_pose_graph *graph, double *poses, int64_t cap, int64_t *n_out, int64_t *indices);
/* size() / loopClosureCount() / getFinalError() + getIterations() (pose_graph.hpp:117-128); any may be NULL */
int icpmi_pose_graph_size(const icpmi_pose_graph *graph, int64_t *num_poses, int64_t *num_loop_closures,
                          icpmi_pose_graph_info *last);

/* A robust loss on the loop-closure edges: GTSAM 4.1+ noiseModel::Robust over the loop factors' diagonal model,
 * restated from the source as published (the reference itself uses the plain Gaussian model, pose_graph.cpp:118-141, and
 * cannot refuse a false closure).  Off by default; with the loss off every call does what it did, bit for bit.
 * The setting is the graph's, not a factor's: it applies to every factor added by add_loop_closure, past and future, at
 * the next optimize().  Priors and odometry factors are never touched.  Per loop factor rw = r / sigma and
 * d = sqrt(sum rw_a^2), `scale` k in whitened units (sigmas):
 *     ICPMI_PG_LOSS_HUBER (1)          w = d <= k ? 1 : k / d              rho = d <= k ? 0.5 d^2 : k (d - 0.5 k)
 *     ICPMI_PG_LOSS_CAUCHY (2)         s = k k,  w = s / (s + d^2)         rho = 0.5 s log1p(d^2 / s)
 *     ICPMI_PG_LOSS_GEMAN_MCCLURE (3)  s = k k,  q = s / (s + d^2), w = q q   rho = 0.5 s d^2 / (s + d^2)
 * No form divides by d except Huber's outer branch, where d > k > 0.
 * Linearisation (Robust::WhitenSystem): A_i, A_j and rw of a loop factor are multiplied by sqrt(w) (q itself for
 * Geman-McClure, sqrt() for the other two); H, g and the linearised error are formed from the scaled values.
 * Error (NoiseModelFactor::error -> Robust::loss): a loop factor contributes rho(d), every other factor 0.5 d^2, for the
 * initial error, every trial's candidate error, the history and final_error.  The LM policy is untouched, and
 * optimize() still starts from the initial estimates: a redescending loss (Cauchy, Geman-McClure) whose scale is below
 * the drift, measured in sigmas, rejects true closures too. */
#define ICPMI_PG_LOSS_NONE 0
#define ICPMI_PG_LOSS_HUBER 1
#define ICPMI_PG_LOSS_CAUCHY 2
#define ICPMI_PG_LOSS_GEMAN_MCCLURE 3
/* A kind outside 0..3, or with a kind other than NONE a scale that is not finite or not > 0, is ICPMI_ERR_ARG with
 * nothing changed.  NONE ignores the scale.  A call that changes the setting clears the optimised state, as adding a
 * factor does; one that repeats it changes nothing. */
int icpmi_pose_graph_set_loop_loss(icpmi_pose_graph *graph, int32_t kind, double scale);
int icpmi_pose_graph_loop_loss(const icpmi_pose_graph *graph, int32_t *kind, double *scale);   /* either may be NULL */
/* Weight w and whitened distance d of every loop closure at the optimised values, in add_loop_closure order: which
 * closures the loss refused.  *n_out receives the number of loop closures; weights and distances may each be NULL;
 * cap < *n_out with a non-NULL array is ICPMI_ERR_CAPACITY.  Only valid while the optimised state of the last
 * optimize() holds, otherwise ICPMI_ERR_ARG.  With the loss off the weights are 1.0 and the distances each closure's
 * residual in sigmas.  One launch and one wait. */
int icpmi_pose_graph_loop_weights(icpmi_pose_graph *graph, double *weights, double *distances, int64_t cap,
                                  int64_t *n_out);

/* Covariances of the optimised poses (GTSAM's Marginals::marginalCovariance / jointMarginalCovariance; not
 * in the reference, which never asks).  H is the Gauss-Newton matrix of the whole graph at the optimised values, with the
 * loop loss' weights and the information edges' R as the optimiser applies them.  For q distinct pose indices, cov
 * receives the 6q x 6q joint marginal covariance, row-major: block (a, b) = (H^-1)[indices[a], indices[b]], in the
 * tangent order (omega, v) of a right perturbation X Exp(xi).  A block does not depend, bit for bit, on the order of the
 * query or on what else is queried.
 * Only valid while the optimised state of the last optimize() holds (nothing added, no loss change since), otherwise
 * ICPMI_ERR_ARG.  Also ICPMI_ERR_ARG: q <= 0, an index without an estimate, an index named twice, and a graph whose H
 * meets a non-positive pivot (no prior: gauge freedom has no covariance).  NULL indices or cov: ICPMI_ERR_NULL.
 * The first call after an optimize() factors H once more at lam = 0 and keeps the factor; later calls only solve. */
int icpmi_pose_graph_marginals(icpmi_pose_graph *graph, const int64_t *indices, int32_t q, double *cov);
/* First-order covariance of the tangent of X_from^-1 X_to: J Sigma J^T with Sigma the joint covariance of (from, to) and
 * J = [-Ad(X_to^-1 X_from), I].  from == to is ICPMI_ERR_ARG; the rest as icpmi_pose_graph_marginals. */
int icpmi_pose_graph_relative_covariance(icpmi_pose_graph *graph, int64_t from, int64_t to, double cov[36]);
/* Squared Mahalanobis distance of a proposed edge `rel` (from -> to, as icpmi_pose_graph_add_loop_closure takes it)
 * against the graph: e = Log(rel^-1 X_from^-1 X_to), *d2 = e^T (Sigma_rel + edge_cov)^-1 e, chi-squared with 6 degrees of
 * freedom for a true closure.  edge_cov is the edge's own 6 x 6 noise covariance; a sum that is not positive definite
 * is ICPMI_ERR_ARG. */
int icpmi_pose_graph_closure_distance(icpmi_pose_graph *graph, int64_t from, int64_t to, const double rel[16],
                                      const double edge_cov[36], double *d2);

/* Between factors weighted by a full 6 x 6 information matrix (GTSAM's noiseModel::Gaussian::Information):
 * an edge stiff where its measurement is well constrained and soft where it is not, instead of six fixed sigmas.  Off by
 * default: a graph that holds no such factor runs the kernels it ran before, bit for bit.
 * `info` is row-major, in the factor's tangent order (omega, v), the inverse covariance of the residual
 * Log(rel^-1 X_from^-1 X_to).  It is checked when the factor is added, on the host: every entry finite, every diagonal
 * entry > 0, |info_ab - info_ba| <= 1e-9 sqrt(info_aa info_bb) (beyond what rounding a 6 x 6 triple product leaves: see
 * csrc/pose_graph_info_host.h), and the upper Cholesky info = R^T R, taken from the upper triangle, succeeds with every
 * pivot finite and > 0.  A matrix that fails is ICPMI_ERR_ARG and the graph is untouched: a semi-definite one (one plane's
 * JtJ) needs a floor first, see icpmi_information_from_icp.  The graph keeps R and whitens by it: rw = R r, A = R J.
 * Estimates, the loop count and the loop edges' loss (icpmi_pose_graph_set_loop_loss, on d = ||R r||) are exactly those
 * of icpmi_pose_graph_add_odometry (with fitness 0) and icpmi_pose_graph_add_loop_closure; icpmi_pose_graph_loop_weights
 * reports d = ||R r|| for such a loop edge.  Diagonal and information factors mix freely in one graph. */
int icpmi_pose_graph_add_odometry_information(icpmi_pose_graph *graph, int64_t from, int64_t to, const double rel[16],
                                              const double info[36]);
int icpmi_pose_graph_add_loop_closure_information(icpmi_pose_graph *graph, int64_t from, int64_t to,
                                                  const double rel[16], const double info[36]);
/* The information of an edge from the normal matrix of the point-to-plane registration that measured it.  Pure host
 * function, fp64 in a fixed operation order (no context, no device):
 *     info_out = Ad_T^T (JtJ / sigma^2) Ad_T + diag(1 / floor_rotation_sigma^2 x 3, 1 / floor_translation_sigma^2 x 3)
 * with Ad_T = [[R, 0], [t^ R, R]], symmetric by construction.
 * JtJ (row-major 6 x 6, the upper triangle is read) is sum J^T J over the registration's pairs at its result T, with
 * J = [(p x n)^T, n^T] per pair, p the moved source point and n the target normal: the curvature of the cost in ICP's own
 * step, a LEFT perturbation x = [r; t] of T in the target frame, p' = p + r x p + t.  The graph's factor perturbs on the
 * RIGHT, and Exp(x) T = T Exp(Ad_{T^-1} x) to first order, hence the adjoint.  The result is the information of an edge
 * entered as rel = T with from = the target's pose and to = the source's.  For a caller who enters the edge the other
 * way round, rel = T^-1 with from = the source's pose: the same JtJ is already right-frame information, info = JtJ /
 * sigma^2 (+ floors), no adjoint -- pass the identity for T.
 * sigma: the residual noise of one pair in metres, finite and > 0; a caller who wants fewer effective points than rows
 * (neighbouring returns are not independent) folds sqrt(rows / effective) into it.  The floors are 0 (none) or finite and
 * > 0: sigmas of an isotropic prior information added to the diagonal, which keep a rank-deficient JtJ (a single plane,
 * a corridor) positive definite.  Anything else, or a non-finite entry of JtJ or T, is ICPMI_ERR_ARG; a NULL pointer
 * ICPMI_ERR_NULL. */
int icpmi_information_from_icp(const double JtJ[36], const double T[16], double sigma, double floor_rotation_sigma,
                               double floor_translation_sigma, double info_out[36]);

/* Global map: the node's kept filtered scans and what it builds from them with the optimised poses
 * (slam_viz/src/ros/slam_node.cpp):
 *     downsampled_clouds_.push_back(curr)                      :71, :123      icpmi_map_add_frame*
 *     rebuild_recent_clouds (after each successful optimize)   :177-194       icpmi_map_world, first = max(0, frames - 20)
 *     build_final_global_map                                   :196-209       icpmi_map_world, first = 0
 *     rebuild_occupancy_grid: clear, then each frame with its own :223-229    icpmi_map_finish (grid)
 *         pose's translation as the sensor position
 *     publish_global_map once complete: voxel_downsample(       :235-238      icpmi_map_finish (voxel_size)
 *         global_map_points_, 2 * voxel_size)
 * The rows live in one device arena owned by the handle, frame after frame; frame k is the k-th add.  Frames of 0
 * rows are legal.  A call uses frames i < min(frames, n_poses) (the reference's i < downsampled_clouds_.size() &&
 * i < poses_.size()); poses are n_poses row-major 4 x 4 (extra ones are ignored), a NULL array with n_poses > 0 is
 * ICPMI_ERR_NULL and a non-finite entry among the used ones ICPMI_ERR_ARG.  World points are
 * ((x R_a0 + y R_a1) + z R_a2) + t_a, bit for bit those of icpmi_stream_map_update and icpmi_transform_points.
 * The store holds at most 700,000,000 rows: an add past that is ICPMI_ERR_ARG and changes nothing.  The handle uses
 * its context's device and stream, with the same lifetime rules as icpmi_pose_graph: destroy it before its context.
 * Each call waits for the device once (icpmi_map_finish: once for the counts, once more for the published map). */
typedef struct icpmi_map icpmi_map;
int icpmi_map_create(icpmi_ctx *ctx, icpmi_map **out);
void icpmi_map_destroy(icpmi_map *map);
int icpmi_map_add_frame(icpmi_map *map, const double *xyz, int64_t n);           /* n x 3 rows in host memory */
int icpmi_map_add_frame_device(icpmi_map *map, const double *d_xyz, int64_t n);  /* ... in device memory */
/* the filtered scan the last icpmi_stream_push* left resident (too-few-points scans included), device to device;
 * ICPMI_ERR_ARG if there is none */
int icpmi_map_add_stream_frame(icpmi_map *map);
int icpmi_map_size(const icpmi_map *map, int64_t *frames, int64_t *points);      /* either may be NULL */
/* World points of frames [first, min(frames, n_poses)), frame then row order, into out_xyz (host, cap rows; fewer
 * than *n_out is ICPMI_ERR_CAPACITY).  out_xyz may be NULL: only *n_out is set, no device work.
 * rebuild_recent_clouds is first = max(0, frames - 20); build_final_global_map is first = 0. */
int icpmi_map_world(icpmi_map *map, const double *poses, int64_t n_poses, int64_t first, double *out_xyz, int64_t cap,
                    int64_t *n_out);
/* build_final_global_map's tail in one world pass; the global map itself never leaves the device.
 *   grid (may be NULL: the set is untouched): rebuild_occupancy_grid into the context's cell set, which
 *     icpmi_occupancy_cells then reads and later updates merge into.  The rebuilt set replaces the old one only if
 *     the whole call succeeds.  Frames the per-frame path never inserts (the first, too-few-points ones) are in it,
 *     as in the reference.
 *   voxel_size > 0 and map_out not NULL (else skipped): voxel_downsample(global map, voxel_size) into map_out
 *     (map_cap rows; too few is ICPMI_ERR_CAPACITY), *n_map its rows.  The rules of icpmi_voxel_downsample hold: more
 *     than 2^21 voxels on an axis is ICPMI_ERR_ARG.
 * n_map and n_cells may be NULL. */
int icpmi_map_finish(icpmi_map *map, const double *poses, int64_t n_poses, const icpmi_grid_config *grid,
                     double voxel_size, double *map_out, int64_t map_cap, int64_t *n_map, int64_t *n_cells);

/* The kept scans ray-cast into a free / occupied / unknown raster a planner can use.  The reference's
 * cells_to_occupancy_grid_msg (slam_node.cpp:279-297) writes 100 for a hit cell and 0 everywhere else, so it
 * publishes space the LiDAR never saw as free; here that space is unknown.  With the frames, poses and grid of
 * icpmi_map_finish (frames i < min(frames, n_poses), the first and too-few-points ones included):
 *   hits      a row of frame i marks the cell icpmi_map_finish(grid) inserts for it, under the same tests (height
 *             band, 0.5 <= r <= max_range from the frame's translation, a representable quotient).  A row that marks
 *             nothing casts no ray.  The occupied cells are exactly icpmi_map_finish's cell set.
 *   rays      from the frame's sensor cell (floor(t.x / resolution), floor(t.y / resolution)) to each hit cell, the
 *             all-integer Bresenham line in that direction (dx = |x1 - x0|, dy = |y1 - y0|, err = dx - dy; while not at
 *             the hit: carve, e2 = 2 err, if e2 > -dy: err -= dy, x += sx; if e2 < dx: err += dx, y += sy).  The sensor
 *             cell is carved, the hit cell is not; a hit in the sensor's own cell carves nothing.
 *   state     100 a cell in the occupied set, whatever passes through it; 0 a cell carved by any ray of any frame and
 *             not occupied; -1 every other cell.  Unions of sets: no dependence on the order of frames or rows.
 *   raster    nav_msgs/OccupancyGrid's layout: min_x, min_y are the least x and y over the occupied and free cells
 *             less 5 cells, width and height reach 5 cells past the greatest, and cell (x, y) is
 *             data[(y - min_y) * width + (x - min_x)].  No occupied and no free cell: 0 x 0.
 * Limits, each refused with ICPMI_ERR_ARG before any device work, nothing changed: resolution not finite or not
 * positive; R = ceil(max_range / resolution) > ICPMI_RAYCAST_MAX_R (a max_range that is not finite included); a used
 * pose with a non-finite entry; a used frame whose sensor cell is more than 2^31 - 2 - R - 6 in magnitude on an axis;
 * width * height > 2^31 - 1, judged before the rays are cast by the raster's bound (W + 10) * (H + 10), W and H being
 * the spans of the sensor cells of the used frames that hold rows, widened by R + 1 cells on every side (every hit
 * lies within R + 1 cells of its sensor cell).  NULL poses with n_poses > 0, or a NULL grid, is ICPMI_ERR_NULL.
 * Rays are walked in a per-frame window in on-chip memory up to R = ICPMI_RAYCAST_LDS_MAX_R and straight in device
 * memory beyond; the results are the same.
 *   icpmi_map_raycast   builds the raster and keeps it on the device, in a buffer the handle owns; info may be NULL.
 *                       A failed call leaves the previous raster in place.  The context's cell set is not touched.
 *                       Waits for the device twice (the raster's size, the raster); once when no cell is marked.
 *   icpmi_map_raster    sets *info (may be NULL) to the last successful raycast's, all zeros before the first, and, if
 *                       data is not NULL, copies its width * height bytes out (cap bytes; fewer is
 *                       ICPMI_ERR_CAPACITY).  One wait. */
#define ICPMI_RAYCAST_MAX_R 4096
#define ICPMI_RAYCAST_LDS_MAX_R 559
typedef struct {
    int32_t min_x, min_y, width, height;
    double resolution;
    int64_t n_occupied, n_free;
} icpmi_raster_info;
int icpmi_map_raycast(icpmi_map *map, const double *poses, int64_t n_poses, const icpmi_grid_config *grid,
                      icpmi_raster_info *info);
int icpmi_map_raster(icpmi_map *map, int8_t *data, int64_t cap, icpmi_raster_info *info);

/* The same rays counted per cell: how many used frames saw a cell occupied and how many saw through it, and the
 * occupancy probability a planner reads from the two.  In icpmi_map_raycast's raster one return of one frame blocks a
 * cell for good; here a parked car that drove off is outvoted by the later frames that look through it.  The frames
 * (i < min(frames, n_poses)), poses, grid, hit cells, sensor cells and ray walk are exactly icpmi_map_raycast's.  For
 * a used frame i:
 *   H_i       the set of its distinct hit cells
 *   C_i       the set of cells carved by any of its rays, minus H_i: within one scan occupied wins
 * and for a cell c:
 *   hits[c]   = #{i : c in H_i}
 *   misses[c] = #{i : c in C_i}
 * so a frame adds at most 1 to each of a cell's two counts, however many of its rows or rays touch the cell.
 *   probability[c]  -1 if hits + misses == 0; else, with n = hits + misses, (200 hits + n) / (2 n) in integer
 *             division: 100 hits / n rounded half up, the counting model, with no floating point.
 *   bounds    tight over the cells with hits + misses > 0, widened by 5 cells: icpmi_map_raycast's box, since the
 *             observed cells are its occupied and free ones.  Nothing observed: 0 x 0.  The layout of each array is
 *             icpmi_map_raster's: cell (x, y) at [(y - min_y) * width + (x - min_x)].
 * Hence hits > 0 exactly where the raster holds 100; hits == 0 and misses > 0 exactly where it holds 0; both -1
 * elsewhere.  All integer sums: no dependence on the order of frames or rows.
 * Every ICPMI_ERR_ARG and ICPMI_ERR_NULL case of icpmi_map_raycast applies unchanged; in addition more than
 * ICPMI_RAYCOUNT_MAX_FRAMES used frames is ICPMI_ERR_ARG (a count is 16 bits wide).  All are decided before any device
 * work.  Up to R = ICPMI_RAYCOUNT_LDS_MAX_R a frame's two bit windows (carved, hit) live in on-chip memory, beyond in
 * device scratch; the results are the same.
 *   icpmi_map_raycast_counts  builds the three arrays and keeps them on the device, in a buffer the handle owns; info
 *                       may be NULL.  A failed call leaves the previous counts in place.  The context's cell set is
 *                       not touched, and neither is icpmi_map_raster's raster: the two products are independent.
 *                       Waits for the device twice (the arrays' size, the arrays); once when nothing is observed.
 *   icpmi_map_counts    sets *info (may be NULL) to the last successful raycast_counts', all zeros before the first,
 *                       and copies out the arrays that are not NULL (cap cells each; fewer than width * height with
 *                       any array given is ICPMI_ERR_CAPACITY).  One wait.
 * info: n_observed cells have hits + misses > 0; n_hit_cells have hits > 0 (icpmi_map_raycast's n_occupied); max_hits
 * and max_misses are the greatest counts; frames_used is min(frames, n_poses). */
#define ICPMI_RAYCOUNT_MAX_FRAMES 65535      /* counts are uint16: a frame adds at most 1 */
#define ICPMI_RAYCOUNT_LDS_MAX_R 392         /* two bit windows in 160 KiB */
typedef struct {
    int32_t min_x, min_y, width, height;
    double resolution;
    int64_t n_observed, n_hit_cells;
    int32_t max_hits, max_misses, frames_used, pad;
} icpmi_counts_info;
int icpmi_map_raycast_counts(icpmi_map *map, const double *poses, int64_t n_poses, const icpmi_grid_config *grid,
                             icpmi_counts_info *info);
int icpmi_map_counts(icpmi_map *map, uint16_t *hits, uint16_t *misses, int8_t *probability, int64_t cap,
                     icpmi_counts_info *info);

/* The same counts kept while the node drives: a count plane that persists in the handle and moves with the map, so
 * that a call casts only the frames that are new.  The contract is one sentence: icpmi_map_live_update(map, poses,
 * n_poses, grid, info) leaves the handle's live counts byte for byte what icpmi_map_raycast_counts(map, poses, n_poses,
 * grid, ...) would build from the same store; only the cost differs.  The handle remembers the grid, the number of
 * frames it has cast (n_cast) and the 16 doubles of the pose each was cast with.  With used = min(frames, n_poses):
 *   incremental  the grid is bitwise the remembered one, used >= n_cast and the first n_cast poses are bitwise the
 *             remembered ones: frames [n_cast, used) are cast and added to the plane; nothing else is touched.
 *   rebuild   every other case (poses moved by an optimize, fewer poses, another grid, the first call, the first call
 *             after icpmi_map_live_clear or after a call that failed on the device): the plane is zeroed and frames
 *             [0, used) are cast, by icpmi_map_raycast_counts' kernels.
 *   nothing new  used == n_cast and nothing changed: no device work, and the same bytes.
 * The counts are integer sums over sets, so the order frames are added in does not show.
 * The plane is a dense box of 32-bit words, one per cell.  A frame whose (2R + 3)^2 window around its sensor cell
 * leaves the box makes the plane grow: a new zeroed allocation and one device copy, with at least half the box's extent
 * of slack on each side that was crossed, so that over a drive the cells copied are at most 4 x the final plane's; the
 * old buffer is freed after the call's wait.  The slack is memory: the plane may hold up to 3/2 of the used frames' own
 * extent on an axis driven one way, and is not held to the 2^31 - 1 cells the used frames' own box is held to.
 * Every ICPMI_ERR_NULL and ICPMI_ERR_ARG case of icpmi_map_raycast_counts applies, the ICPMI_RAYCOUNT_MAX_FRAMES cap
 * included, decided by the same host code before any device work; such a call leaves *info unwritten and the live
 * state as it was, and the next good call is still incremental.  An ICPMI_ERR_HIP in the middle of a call marks the
 * state invalid: the next call rebuilds.
 *   icpmi_map_live_update  info may be NULL.  One wait for the device (none when nothing was cast).
 *   icpmi_map_live_counts  sets *info (may be NULL) to the last successful update's, all zeros before the first and
 *                       after a clear, and copies out the arrays that are not NULL: layout, cap and NULL rules of
 *                       icpmi_map_counts, info->counts.width * height cells each.  One wait.
 *   icpmi_map_live_clear   forgets the cast frames: the next update casts every used frame again.
 * Neither call touches icpmi_map_counts' arrays, icpmi_map_raster's raster or the context's cell set, and neither
 * icpmi_map_raycast_counts nor icpmi_map_raycast touches the live counts.  icpmi_map_world_static and
 * icpmi_map_finish_static (below) do: each begins with exactly this update.
 * info: counts is exactly what icpmi_map_raycast_counts would report; frames_cast the frames this call cast (0 when
 * nothing was new); rebuilt 1 when remembered frames were discarded and cast again; moved 1 when the plane was
 * reallocated and its words copied in this call; plane_* the plane's box in cells (0 x 0: no plane). */
typedef struct {
    icpmi_counts_info counts;
    int64_t frames_cast;
    int32_t rebuilt;
    int32_t moved;
    int32_t plane_x0, plane_y0, plane_w, plane_h;
} icpmi_live_info;
int icpmi_map_live_update(icpmi_map *map, const double *poses, int64_t n_poses, const icpmi_grid_config *grid,
                          icpmi_live_info *info);
int icpmi_map_live_counts(icpmi_map *map, uint16_t *hits, uint16_t *misses, int8_t *probability, int64_t cap,
                          icpmi_live_info *info);
int icpmi_map_live_clear(icpmi_map *map);

/* Ground segmentation of a scan in its SENSOR frame (not in the reference, which names it as future work,
 * README.md:304), and the occupancy products built from a scan's obstacle rows instead of a band on world z.
 * A polar grid of n_rings x n_sectors bins covers [min_range, max_range].  fp64, unfused, in the order written
 * (scripts/ground_ref.py restates it byte for byte):
 *   bin      range = sqrt(x*x + y*y), angle = atan2(y, x) + pi; ring = (int)((range - min_range) / ring_size) and
 *            sector = (int)(angle / sector_size), each clamped to its last index, with ring_size = (max_range -
 *            min_range) / n_rings and sector_size = 2 pi / n_sectors.  A row with a non-finite coordinate, or with
 *            range < min_range or range > max_range, enters no bin and is ICPMI_GROUND_IGNORED.
 *   pass 1   zmin[bin] = the least z of the bin's rows (independent of the row order).
 *   walk     per sector, outward: gz = -sensor_height, gr = 0; at ring r with centre rc = min_range + (r + 0.5) *
 *            ring_size, a bin that holds rows is accepted if fabs(zmin - gz) <= step_tol + max_slope * (rc - gr), and
 *            then gz = zmin, gr = rc; in every case ground_z[bin] = gz.
 *   pass 2   h = z - ground_z[bin]: ICPMI_GROUND_GROUND if h <= height_tol, else ICPMI_GROUND_OBSTACLE if clear_min <= h
 *            <= clear_max, else ICPMI_GROUND_IGNORED.
 * icpmi_ground_segment labels n rows in host memory, icpmi_ground_segment_device n rows in device memory; the outputs
 * are host memory in both: labels (n bytes), height (n doubles: h, NaN for a row that entered no bin; may be NULL),
 * ground_z (n_rings * n_sectors doubles, ring-major; may be NULL), info (may be NULL; bins_accepted counts the bins
 * whose own minimum was taken as ground).  n == 0 is legal (xyz and labels may then be NULL).  One wait.
 * ICPMI_ERR_ARG, before any device work and with nothing written: a config field that is not finite; n_rings < 1 or
 * n_sectors < 1; n_rings * n_sectors > ICPMI_GROUND_MAX_BINS (the bins live in one compute unit's LDS); min_range < 0
 * or max_range <= min_range; a negative max_slope, step_tol or height_tol; clear_max < clear_min. */
#define ICPMI_GROUND_OBSTACLE 0
#define ICPMI_GROUND_GROUND 1
#define ICPMI_GROUND_IGNORED 2
#define ICPMI_GROUND_MAX_BINS 20400
typedef struct {
    int32_t n_rings, n_sectors;
    double min_range, max_range;
    double sensor_height;            /* the prior: the ground lies this far below the sensor */
    double max_slope, step_tol;
    double height_tol;
    double clear_min, clear_max;     /* the clearance band of an obstacle, over the ground */
} icpmi_ground_config;
typedef struct {
    int64_t n_ground, n_obstacle, n_ignored, bins_accepted;
} icpmi_ground_info;
void icpmi_ground_config_default(icpmi_ground_config *cfg); /* 80, 180, 0.5, 80.5, 1.73, 0.15, 0.1, 0.2, 0.3, 2.0 */
int icpmi_ground_segment(icpmi_ctx *ctx, const double *xyz, int64_t n, const icpmi_ground_config *cfg, uint8_t *labels,
                         double *height, double *ground_z, icpmi_ground_info *info);
int icpmi_ground_segment_device(icpmi_ctx *ctx, const double *d_xyz, int64_t n, const icpmi_ground_config *cfg,
                                uint8_t *labels, double *height, double *ground_z, icpmi_ground_info *info);

/* Motion compensation (deskew) of a scan in its sensor frame (csrc/deskew.h; not in the reference, which
 * takes every scan as a snapshot from one pose).  A spinning sensor measures row i at tau_i in [0, 1] of its sweep while
 * it moves; with the motion over one whole sweep given as a twist xi = (omega, v) in the sensor frame (the tangent
 * order of the pose graph), pose(tau) = pose(t_ref) Exp((tau - t_ref) xi), and row i becomes
 *     p'_i = Exp(s_i xi) p_i = R(s_i) p_i + t(s_i),   s_i = tau_i - t_ref:
 * the scan as a sensor standing at pose(t_ref) would have seen it.  With theta = |omega|, a = omega / theta, K = hat(a):
 *     R(s) = I + sin(s theta) K + (1 - cos(s theta)) K^2
 *     t(s) = s v + ((1 - cos(s theta)) / theta) (a x v) + ((s theta - sin(s theta)) / theta) (a x (a x v))
 * and for theta < 1e-10 R = I, t = s v.  fp64, unfused, in the order csrc/deskew.h states (scripts/deskew_ref.py restates
 * it byte for byte while |s| theta < pi/4; from there on the device library's sincos is used, a few ulp from libm's).
 * A row with a non-finite coordinate or time, a row with tau_i == t_ref, and every row under a twist of six zeros pass
 * through unchanged in every bit.
 *   time_source  ICPMI_DESKEW_TIMES: `times` holds n doubles, tau_i as given.
 *                ICPMI_DESKEW_AZIMUTH: tau_i = frac(direction * (atan2(y, x) - azimuth_start) / 2 pi); `times` is not
 *                read.  What a KITTI .bin, which carries no times, gets.
 *   t_ref        the moment of the sweep whose pose the deskewed scan is registered as: 0.5, mid-sweep, by default.
 * icpmi_deskew works on host memory (one wait); icpmi_deskew_device on device memory, queued on the context's stream
 * with no wait of its own.  out_xyz may be xyz.  n == 0 is ICPMI_OK.  Decided before any device work, with nothing
 * written and a text in icpmi_last_error -- ICPMI_ERR_ARG: a twist entry, t_ref or azimuth_start that is not finite;
 * t_ref outside [0, 1]; direction not +1 or -1; an unknown time_source; n < 0 -- ICPMI_ERR_NULL: cfg, xyz or out_xyz
 * NULL with n > 0, or ICPMI_DESKEW_TIMES with times NULL and n > 0.  reserved[] is ignored.
 * icpmi_deskew_twist: twist = Log(delta), the SE(3) log of a relative pose (row-major 4 x 4), with the pose graph's
 * formulas and small-angle forms: the twist of a sweep under constant velocity, from the previous frame's delta.  Host
 * only: no context, no device.  A non-finite entry is ICPMI_ERR_ARG. */
#define ICPMI_DESKEW_TIMES 0
#define ICPMI_DESKEW_AZIMUTH 1
typedef struct {
    double twist[6];        /* (omega, v) over one whole sweep, in the sensor frame */
    double t_ref;           /* in [0, 1] */
    int32_t time_source;    /* ICPMI_DESKEW_* */
    int32_t direction;      /* +1: the azimuth grows with time (counter-clockwise); -1: clockwise */
    double azimuth_start;   /* the azimuth at tau = 0 [rad] */
    double reserved[4];
} icpmi_deskew_config;
void icpmi_deskew_config_default(icpmi_deskew_config *cfg); /* zero twist, 0.5, ICPMI_DESKEW_TIMES, +1, -pi */
int icpmi_deskew(icpmi_ctx *ctx, const double *xyz, const double *times, int64_t n, const icpmi_deskew_config *cfg,
                 double *out_xyz);
int icpmi_deskew_device(icpmi_ctx *ctx, const double *d_xyz, const double *d_times, int64_t n,
                        const icpmi_deskew_config *cfg, double *d_out_xyz);
int icpmi_deskew_twist(const double delta[16], double twist[6]);
/* Deskew in the odometry stream: while a config is set (NULL turns it off; off after icpmi_create), icpmi_stream_push
 * and icpmi_stream_push_host first deskew the raw scan under it into a buffer of the context, on the context's stream
 * and with no additional wait, and filter and register that: bit for bit icpmi_deskew followed by the same push with
 * deskew off.  The caller sets the twist before each push (it owns the gate and the pose: icpmi_deskew_twist of its last
 * delta is the constant-velocity choice).  The stream has no times: the config's time_source must be
 * ICPMI_DESKEW_AZIMUTH (anything else is ICPMI_ERR_ARG, as are the cases of icpmi_deskew).  The setting survives
 * icpmi_stream_reset.  While it is set icpmi_stream_push_file and icpmi_stream_prefetch_file return ICPMI_ERR_ARG: the
 * prefetch worker filters the next file before this frame's delta exists.  With deskew off every stream call is bit for
 * bit what it is without this function. */
int icpmi_stream_set_deskew(icpmi_ctx *ctx, const icpmi_deskew_config *cfg);

/* icpmi_map_set_ground(map, cfg): while a config is set (NULL turns it off; off after icpmi_map_create),
 * icpmi_map_finish's cell set, icpmi_map_raycast, icpmi_map_raycast_counts and icpmi_map_live_update take as a frame's
 * hits exactly its ICPMI_GROUND_OBSTACLE rows.  The grid's world-z band is not applied; every other test stays (0.5 <=
 * r <= max_range from the frame's translation, a representable cell).  A row with another label marks nothing and
 * casts no ray, as a row outside the band does without ground.  Stated as an equivalence: each product, its info
 * included, is byte for byte that of a second store holding, frame by frame and in order, only the OBSTACLE rows, run
 * without ground and with height_min = -DBL_MAX, height_max = DBL_MAX.  icpmi_map_world, the published voxel map of
 * icpmi_map_finish and the loop-closure store are not affected.  The labels are a property of a frame's rows alone, so
 * they survive an optimize: they are formed at the start of the first of those calls that needs them, for every frame
 * not yet labelled, in one launch and one wait of its own (it tells the host which frames hold an OBSTACLE row), and
 * kept until icpmi_map_set_ground is called again.  Every call to it, with the same config or another, also invalidates
 * the live counts: the next icpmi_map_live_update rebuilds.  A bad config is ICPMI_ERR_ARG and changes nothing.
 * With ground off every call is bit for bit what it is without this function.
 * icpmi_map_ground_labels: *n_out = the frame's rows; labels (may be NULL with cap 0: the size alone) receives its
 * cached bytes, formed first if need be; a cap below the rows is ICPMI_ERR_CAPACITY; without a ground config, or with a
 * frame out of range, ICPMI_ERR_ARG. */
int icpmi_map_set_ground(icpmi_map *map, const icpmi_ground_config *cfg);
int icpmi_map_ground_labels(icpmi_map *map, int64_t frame, uint8_t *labels, int64_t cap, int64_t *n_out);

/* The static map: icpmi_map_world and the published map of icpmi_map_finish without the rows whose cells the counts
 * outvote (csrc/static_map.h; not in the reference, whose map keeps every return of everything that moved
 * while the node drove).  For the used frames i < used = min(frames, n_poses) and the caller's grid, let hits[c],
 * misses[c] and probability[c] be exactly what icpmi_map_raycast_counts(map, poses, n_poses, grid) defines.
 *   A row of used frame i VOTES iff it marks a cell c under the rules the counts use: grid_cell_key of its world
 *   point with frame i's translation as the sensor and, while icpmi_map_set_ground is on, additionally its label is
 *   OBSTACLE and the band is open.  With n = hits[c] + misses[c] a row's label is
 *     0  kept, does not vote: ground rows, rows out of band or ring, non-finite rows, an unrepresentable quotient
 *     1  kept, votes
 *     2  dropped: the row votes, n >= rule.min_observations and probability[c] < rule.min_probability
 *   probability[c] = (200 hits[c] + n) / (2 n) in integer division.  A lookup that finds n == 0, or a cell outside
 *   the plane's box, keeps the row with label 1 (it cannot happen for a voting row).  min_probability == 0 drops
 *   nothing.  All integer: no dependence on the order of frames, rows or threads.
 * The vote is two-dimensional: which rows vote is decided by the grid's band on world z, or by the ground labels.  With
 * the default band (0.3 .. 2.0) and the sensor as the origin of z, a car whose roof lies below z = 0.3 never votes and is
 * never dropped: give a band that holds what may move, or set a ground config, under which every OBSTACLE row votes.
 * rule: 0 <= min_probability <= 100, min_observations >= 1, reserved == 0; anything else is ICPMI_ERR_ARG, a NULL rule
 * ICPMI_ERR_NULL.
 * Where the counts come from: both calls first bring the handle's live counts up to date, by the host decision and the
 * kernels of icpmi_map_live_update(map, poses, n_poses, grid) and with its effect on the live state (incremental,
 * rebuild or nothing new; info->live reports which), and label against the live plane: a node that publishes a static
 * cloud every few frames casts only the new frames.  Every ICPMI_ERR_NULL and ICPMI_ERR_ARG case of
 * icpmi_map_live_update applies unchanged, the ICPMI_RAYCOUNT_MAX_FRAMES cap included; those and the rule's are decided
 * before any device work and leave *info unwritten and the labels and the live state as they were.  icpmi_map_counts'
 * arrays, icpmi_map_raster's raster and the context's cell set are never touched.
 *   icpmi_map_world_static   icpmi_map_world restricted to the kept rows: the world points of the rows of frames
 *                       [first, used) whose label is not 2, frame then row order (a stable compaction), each bit for bit
 *                       the point icpmi_map_world writes for that row.  *n_out their number; out_xyz may be NULL: only
 *                       *n_out is set, which still needs the labels and so the device.  cap < *n_out with out_xyz given
 *                       is ICPMI_ERR_CAPACITY.  The labels are formed for all used frames [0, used) whatever first is.
 *                       Waits for the device for the counts (icpmi_map_live_update's wait), for the labels' totals, and
 *                       for the points.
 *   icpmi_map_finish_static  icpmi_map_finish's published-map half over the kept rows of all used frames:
 *                       voxel_downsample(kept world rows, voxel_size) into map_out (map_cap rows), *n_map its rows, under
 *                       the rules and errors of icpmi_map_finish; voxel_size <= 0 or map_out NULL skips the filter (the
 *                       labels and *info are formed all the same).  The context's cell set is not touched.
 *   icpmi_map_static_labels  one frame's label bytes as the last call of either of the two that got as far as the
 *                       labels left them (a call that then fails with ICPMI_ERR_CAPACITY has), in a buffer the handle
 *                       owns: *n_out = the frame's rows; labels may be NULL (the size alone); a cap below the rows is
 *                       ICPMI_ERR_CAPACITY; before any such call, or for a frame that call did not use, ICPMI_ERR_ARG.
 * info (may be NULL): rows = the used frames' rows; voting those with label 1 or 2; dropped those with label 2; kept =
 * rows - dropped, all over the used frames [0, used) whatever first is; live = what icpmi_map_live_update reports. */
#define ICPMI_STATIC_MIN_PROBABILITY_DEFAULT 50
#define ICPMI_STATIC_MIN_OBSERVATIONS_DEFAULT 3
typedef struct {
    int32_t min_probability;    /* a voting row is dropped if its cell's probability is below this */
    int32_t min_observations;   /* ... and the cell was observed (hit or seen through) by at least this many frames */
    int64_t reserved;           /* 0 */
} icpmi_static_rule;
typedef struct {
    int64_t rows, voting, dropped, kept;
    icpmi_live_info live;
} icpmi_static_info;
int icpmi_map_world_static(icpmi_map *map, const double *poses, int64_t n_poses, const icpmi_grid_config *grid,
                           const icpmi_static_rule *rule, int64_t first, double *out_xyz, int64_t cap, int64_t *n_out,
                           icpmi_static_info *info);
int icpmi_map_finish_static(icpmi_map *map, const double *poses, int64_t n_poses, const icpmi_grid_config *grid,
                            const icpmi_static_rule *rule, double voxel_size, double *map_out, int64_t map_cap,
                            int64_t *n_map, icpmi_static_info *info);
int icpmi_map_static_labels(icpmi_map *map, int64_t frame, uint8_t *labels, int64_t cap, int64_t *n_out);

/* Loop-closure detection over a global map's kept scans (slam::LoopClosureDetector, core/loop_closure.hpp:41-148),
 * with its database on the device: an entry is a store frame with a label (the node's frame_idx).  Each entry's
 * Scan Context descriptor lives in device memory; its rows stay in the store and are never copied to the host.
 *   icpmi_loop_add_frame      addFrame (:53-60): entry = store frame, labelled frame_idx.  No device work: the
 *                             descriptors of the entries added since the last detect are formed at its start, in one
 *                             launch, bit for bit those of icpmi_scan_context on the same rows.
 *   icpmi_loop_detect         detect (:66-126) for the newest entry q: every older entry i with
 *                             label[q] - label[i] >= frame_gap and a distance (bit for bit icpmi_scan_context_distances)
 *                             below sc_distance_threshold is a candidate; the candidates, by distance then entry, are
 *                             verified with icp_point_to_plane(query rows, candidate rows) (30 iterations, tolerance
 *                             1e-6, min_error 1e-9, identity start) until max_candidates are accepted (converged and
 *                             final_error < icp_fitness_threshold).  Up to min(max_candidates - accepted,
 *                             ICPMI_MAX_BATCH) of them run side by side, as in icpmi_align_batch.  The results are those
 *                             of the host detector over the same clouds.  One wait for the candidates, then the
 *                             verifications' own.  Fewer than two entries: *n_out = 0.  A cap of max_candidates always
 *                             suffices; fewer than the results is ICPMI_ERR_CAPACITY.  A context with a communicator
 *                             is refused (ICPMI_ERR_ARG); a verification's error is returned as icpmi_align_batch
 *                             returns it.
 *   icpmi_loop_descriptor     entry's 20 x 60 descriptor (row-major) into desc_out; forms any pending ones first.
 *   icpmi_loop_clear          drops every entry; the store is untouched.
 *   icpmi_loop_set_yaw_guess  on != 0 (off at creation; not in the reference): detect keeps the column shift that
 *                             attained each candidate's distance (icpmi_scan_context_distances_shift) and starts its
 *                             verification from icpmi_sc_shift_transform(shift) instead of from the identity, so a
 *                             place revisited with another heading verifies.  Candidates, their order (distance, then
 *                             entry; the shift never enters it) and the distances are unchanged; the result's
 *                             transform is the registration's, which includes the start.  Entries and descriptors
 *                             are untouched; takes effect at the next detect.
 *   icpmi_loop_last_shifts    the shifts the last detect's results started from, in result order: *n_out = the number
 *                             of results (shifts may be NULL with cap 0; a cap below it is ICPMI_ERR_CAPACITY); each is
 *                             -1 when that detect ran with the guess off.
 *   icpmi_loop_set_gate       max_distance > 0 (0: off, as at creation; not in the reference): detect's verifications
 *                             run behind that correspondence-distance gate (icpmi_align_gated), so a place revisited
 *                             a lane aside -- scans that overlap only partly -- verifies; icp_fitness is then the RMS
 *                             over the kept rows.  Composes with the yaw guess; candidates and their order are
 *                             unchanged; takes effect at the next detect.  Negative or non-finite: ICPMI_ERR_ARG.
 *   icpmi_loop_last_pairs     the rows each of the last detect's results kept in its last pass, in result order, as
 *                             icpmi_loop_last_shifts returns the shifts; each is -1 when that detect ran ungated.
 *   icpmi_loop_set_robust     kind ICPMI_ROBUST_* with scale finite and > 0 (kind 0: off, as at creation, scale ignored;
 *                             not in the reference): detect's verifications run under those row weights
 *                             (icpmi_align_robust); icp_fitness is then the weighted RMS, which reads lower than the
 *                             plain one against icp_fitness_threshold.  Composes with icpmi_loop_set_gate and the yaw
 *                             guess; candidates and their order are unchanged; takes effect at the next detect.
 *                             Anything else: ICPMI_ERR_ARG.
 *   icpmi_loop_last_weights   the weight sum of each of the last detect's results' last pass, in result order, as
 *                             icpmi_loop_last_pairs returns the pairs; each is -1 when that detect ran without weights.
 *   icpmi_loop_set_gicp       epsilon with 0 < epsilon <= 1 (0: off, as at creation; not in the reference): detect's
 *                             verifications are plane-to-plane registrations (icpmi_align_gicp with
 *                             ICPMI_GICP_FORM_SMALL and max_distance = the loop's gate, 0 for none); icp_fitness is then
 *                             that call's error, in metres.  Composes with icpmi_loop_set_gate and the yaw guess;
 *                             exclusive with icpmi_loop_set_robust: whichever setter would turn both on returns
 *                             ICPMI_ERR_ARG and leaves the state as it was.  While it is on icpmi_loop_last_pairs
 *                             reports the kept rows, gate or not, and icpmi_loop_set_information keeps working with
 *                             weight = pairs.  Takes effect at the next detect.  Anything else: ICPMI_ERR_ARG.
 *   icpmi_loop_set_information   sigma finite and > 0 with floors 0 or finite and > 0 (sigma 0: off, as at creation, the
 *                             floors ignored; not in the reference): detect keeps, per result, the information matrix
 *                             icpmi_information_from_icp makes of that verification's own normal matrix
 *                             (icpmi_last_normal_matrix) and transform with these three arguments -- the edge's weight
 *                             for icpmi_pose_graph_add_loop_closure_information(match, query, transform, info).  Costs
 *                             a detect nothing on the device.  Composes with gate, weights and yaw guess; takes effect
 *                             at the next detect.  Anything else: ICPMI_ERR_ARG.
 *   icpmi_loop_last_information   36 doubles (row-major 6 x 6) per result of the last detect, in result order, as
 *                             icpmi_loop_last_pairs returns the pairs (cap counts matrices); none (*n_out 0) when that
 *                             detect ran with the setting off.
 * A store frame or an entry out of range is ICPMI_ERR_ARG and changes nothing.  The handle uses its map's context and
 * stream: destroy it before its map, and the map before the context. */
typedef struct icpmi_loop icpmi_loop;
typedef struct {
    int32_t frame_gap;             /* loop_closure.hpp:15 */
    int32_t max_candidates;        /* :18 */
    double sc_distance_threshold;  /* :16 */
    double icp_fitness_threshold;  /* :17 */
} icpmi_loop_config;
typedef struct {                   /* LoopClosureResult, :25-31 */
    int32_t query_frame, match_frame;
    double transform[16];          /* row-major, maps the query's rows onto the match's */
    double scan_context_distance;
    double icp_fitness;
} icpmi_loop_result;
void icpmi_loop_config_default(icpmi_loop_config *cfg); /* :14-19: 50, 3, 0.25, 0.3 */
int icpmi_loop_create(icpmi_map *map, const icpmi_loop_config *cfg, icpmi_loop **out);
void icpmi_loop_destroy(icpmi_loop *loop);
int icpmi_loop_add_frame(icpmi_loop *loop, int64_t store_frame, int32_t frame_idx);
int icpmi_loop_detect(icpmi_loop *loop, icpmi_loop_result *out, int64_t cap, int64_t *n_out);
int icpmi_loop_descriptor(icpmi_loop *loop, int64_t entry, double *desc_out /* 1200 */);
int icpmi_loop_size(const icpmi_loop *loop, int64_t *entries);
int icpmi_loop_clear(icpmi_loop *loop);
int icpmi_loop_set_yaw_guess(icpmi_loop *loop, int32_t on);
int icpmi_loop_last_shifts(const icpmi_loop *loop, int32_t *shifts, int64_t cap, int64_t *n_out);
int icpmi_loop_set_gate(icpmi_loop *loop, double max_distance);
int icpmi_loop_last_pairs(const icpmi_loop *loop, int64_t *pairs, int64_t cap, int64_t *n_out);
int icpmi_loop_set_robust(icpmi_loop *loop, int32_t kind, double scale);
int icpmi_loop_last_weights(const icpmi_loop *loop, double *weights, int64_t cap, int64_t *n_out);
int icpmi_loop_set_gicp(icpmi_loop *loop, double epsilon);
int icpmi_loop_set_information(icpmi_loop *loop, double sigma, double floor_rotation_sigma, double floor_translation_sigma);
int icpmi_loop_last_information(const icpmi_loop *loop, double *info, int64_t cap, int64_t *n_out);

/* Scan-to-local-map odometry (not in the reference node, which registers each scan against the one before it,
 * slam_node.cpp:132-138): a sliding voxel map of the recent scans in one frame, kept on the device, as the
 * registration target.  The table holds sorted unique 63-bit voxel keys and one fp64 point per key, at most `capacity`
 * rows (64 bytes of device memory per row of capacity: two buffers of key + point).  Its rules, which
 * scripts/local_map_ref.py restates in numpy and reproduces byte for byte:
 *   world point  of a scan row under `pose` (row-major 4 x 4): ((x R_a0 + y R_a1) + z R_a2) + t_a per axis a, no FMA.
 *   key          per axis c = (long long)floor(p / voxel_size), accepted in [-2^20, 2^20);
 *                key = (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20): absolute, the table outlives a call.
 *   range        d2 = (dx*dx + dy*dy) + dz*dz against the pose's translation; in range when d2 <= max_range * max_range.
 *   dropped row  a coordinate of its world point is not finite, a cell is outside the key range, or it is out of range.
 *   add(scan, pose):  residents out of range of this pose leave (evicted); among the rows not dropped, the lowest scan
 *                row of each voxel is inserted if its key is not a surviving resident's (so a voxel whose resident was
 *                evicted is taken again by this scan's row); the other rows of a held voxel are merged away; survivors
 *                and insertions are the new table, sorted by key.  inserted + dropped + merged == n, and
 *                rows == rows before - evicted + inserted.
 *   capacity     an add whose result would exceed `capacity` rows returns ICPMI_ERR_CAPACITY and leaves the table as it was.
 * max_range must cover the sensor's range: a scan whose far rows have no counterpart in the map loses the track.
 *   icpmi_local_map_add*          n == 0 is legal and evicts only.  info may be NULL.  One wait for the device.  Behind
 *                             it the new table is prepared as a registration target (search structure, normals) on the
 *                             context's stream, without waiting: the next icpmi_local_map_register* finds it in place
 *                             unless another call on the context prepared a search in between, in which case register
 *                             prepares it again -- the results are the same bits either way.
 *   icpmi_local_map_add_stream_frame  the scan is the filtered one the context's last icpmi_stream_push* left resident
 *                             (ICPMI_ERR_ARG without one).
 *   icpmi_local_map_points        *n_out = rows; out_xyz (rows x 3) and out_keys (rows), each may be NULL, are filled when
 *                             cap >= rows (ICPMI_ERR_CAPACITY when one is given and cap is less).
 *   icpmi_local_map_register*     icp_point_to_plane(source = scan, target = the table's points, cfg): bit for bit
 *                             icpmi_align_device on the same two arrays, with whichever engine ICPMI_SEARCH_AUTO picks
 *                             for the table's size.  cfg->initial_transform is the guess in the map's frame and
 *                             result->transformation the scan's pose in it.  An empty table is ICPMI_ERR_EMPTY_TARGET.
 *   icpmi_local_map_register_robust*  the same through icpmi_align_robust_device (rule and info as there).
 *   icpmi_local_map_clear         empties the table; the configuration stays.
 * ICPMI_ERR_ARG: voxel_size or max_range not finite or <= 0, capacity < 1 or > 2^27, a pose entry that is not finite,
 * n < 0 or above 2^27.  ICPMI_ERR_NULL: any pointer above not marked optional.  The handle uses its context's stream and
 * workspace: destroy it before the context. */
typedef struct icpmi_local_map icpmi_local_map;
typedef struct {
    double voxel_size;  /* 0.5 */
    double max_range;   /* 100.0: must cover the sensor's range */
    int64_t capacity;   /* rows; 1 << 20 */
} icpmi_local_map_config;
typedef struct {
    int64_t rows;       /* of the table after the add */
    int64_t inserted, evicted, dropped, merged;
} icpmi_local_map_info;
void icpmi_local_map_config_default(icpmi_local_map_config *cfg);
int icpmi_local_map_create(icpmi_ctx *ctx, const icpmi_local_map_config *cfg, icpmi_local_map **out);
void icpmi_local_map_destroy(icpmi_local_map *map);
int icpmi_local_map_clear(icpmi_local_map *map);
int icpmi_local_map_add(icpmi_local_map *map, const double *xyz, int64_t n, const double pose[16], icpmi_local_map_info *info);
int icpmi_local_map_add_device(icpmi_local_map *map, const double *d_xyz, int64_t n, const double pose[16],
                               icpmi_local_map_info *info);
int icpmi_local_map_add_stream_frame(icpmi_local_map *map, const double pose[16], icpmi_local_map_info *info);
int icpmi_local_map_size(const icpmi_local_map *map, int64_t *rows);
int icpmi_local_map_points(icpmi_local_map *map, double *out_xyz, uint64_t *out_keys, int64_t cap, int64_t *n_out);
int icpmi_local_map_register(icpmi_local_map *map, const double *xyz, int64_t n, const icpmi_config *cfg, icpmi_result *result,
                             double *error_history, int32_t history_cap);
int icpmi_local_map_register_device(icpmi_local_map *map, const double *d_xyz, int64_t n, const icpmi_config *cfg,
                                    icpmi_result *result, double *error_history, int32_t history_cap);
int icpmi_local_map_register_robust(icpmi_local_map *map, const double *xyz, int64_t n, const icpmi_config *cfg,
                                    const icpmi_robust *rule, icpmi_result *result, icpmi_robust_info *info,
                                    double *error_history, int32_t history_cap);
int icpmi_local_map_register_robust_device(icpmi_local_map *map, const double *d_xyz, int64_t n, const icpmi_config *cfg,
                                           const icpmi_robust *rule, icpmi_result *result, icpmi_robust_info *info,
                                           double *error_history, int32_t history_cap);

/* profiling */
int icpmi_reset_profile(icpmi_ctx *ctx);
int icpmi_get_profile(icpmi_ctx *ctx, icpmi_profile *out);

#ifdef __cplusplus
}
#endif
#endif
