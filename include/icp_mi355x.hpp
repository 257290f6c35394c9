// icp_mi355x.hpp -- header-only C++17 host mirror of the reference's registration API on
// top of the C ABI (icp_mi355x.h).  Eigen-free: the reference's types are restated with
// plain storage so a caller without Eigen can use the same names and call shapes:
//
//   reference (slam_viz/include/slam_viz/core/)          here (namespace icp_mi355x)
//   slam::PointCloud            types.hpp:15-61          PointCloud   (row-major N x 3 fp64)
//   slam::Transformation        types.hpp:74-136         Transformation (row-major 4x4)
//   slam::ICPConfig             types.hpp:143-148        ICPConfig
//   slam::ICPResult             types.hpp:155-164        ICPResult
//   slam::icp_point_to_plane    icp.hpp:157-161          icp_point_to_plane
//   slam::KDTree                kdtree.hpp:18-186        KDTree (nearest, nearest_batch)
//   slam::NearestNeighborSearch kdtree.hpp:193-221       NearestNeighborSearch (find_correspondences)
//   slam::estimate_normals      icp.hpp:23-67            estimate_normals
//   slam::solve_point_to_plane  icp.hpp:89-144           solve_point_to_plane
//   (north_star wording)                                 ICP::align
//   slam::ScanContext           scan_context.hpp:44-142      ScanContext (compute, distance), scan_context_distances
//   slam::LoopClosureConfig / LoopClosureResult / LoopClosureDetector
//                               loop_closure.hpp:14-148      LoopClosureConfig, LoopClosureResult, LoopClosureDetector
//   SlamNode::process_frame, registration and map side   OdometryStream (push, map_update)
//     (slam_viz/src/ros/slam_node.cpp:118-157)
//   OccupancyGridConfig / GridCell / update_occupancy_grid / cells_to_occupancy_grid_msg
//     (slam_viz/include/slam_viz/ros/slam_node.hpp:35-58, slam_node.cpp:211-221,279-297)
//                                                        OccupancyGridConfig, GridCell, OccupancyGrid
//   slam::PoseGraphConfig / slam::PoseGraph
//                               pose_graph.hpp:22-147        PoseGraphConfig, PoseGraph (device Levenberg-Marquardt)
//   downsampled_clouds_ / rebuild_recent_clouds / build_final_global_map / rebuild_occupancy_grid / publish_global_map
//     (slam_node.cpp:71,123,187-209,223-229,235-238)       GlobalMap (kept scans in device memory)
//
// A caller that already has Eigen and the reference's own types uses
// slam_icp_adapter.hpp instead, which keeps slam::icp_point_to_plane's exact signature.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "icp_mi355x.h"

namespace icp_mi355x {

class PointCloud { // types.hpp:15-61
public:
    PointCloud() = default;
    explicit PointCloud(std::vector<double> xyz) : xyz_(std::move(xyz))
    {
        if (xyz_.size() % 3) throw std::invalid_argument("PointCloud: size not a multiple of 3");
    }
    PointCloud(const double *xyz, std::size_t n) : xyz_(xyz, xyz + 3 * n) {}
    const double *data() const { return xyz_.data(); }
    double *data() { return xyz_.data(); }
    std::size_t size() const { return xyz_.size() / 3; }
    bool empty() const { return xyz_.empty(); }
    const double *row(std::size_t i) const { return &xyz_[3 * i]; }
    std::array<double, 3> centroid() const
    {
        std::array<double, 3> c{0, 0, 0};
        for (std::size_t i = 0; i < size(); ++i)
            for (int a = 0; a < 3; ++a) c[a] += xyz_[3 * i + a];
        if (size())
            for (int a = 0; a < 3; ++a) c[a] /= static_cast<double>(size());
        return c;
    }
    PointCloud copy() const { return PointCloud(xyz_); }

private:
    std::vector<double> xyz_;
};

class Transformation { // types.hpp:74-136, row-major storage
public:
    Transformation() { m_ = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}; }
    explicit Transformation(const std::array<double, 16> &row_major) : m_(row_major) {}
    static Transformation identity() { return Transformation(); }
    static Transformation from_rt(const std::array<double, 9> &R, const std::array<double, 3> &t)
    {
        Transformation T;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) T.m_[4 * i + j] = R[3 * i + j];
            T.m_[4 * i + 3] = t[i];
        }
        return T;
    }
    const std::array<double, 16> &matrix() const { return m_; }
    double operator()(int r, int c) const { return m_[4 * r + c]; }
    std::array<double, 3> t() const { return {m_[3], m_[7], m_[11]}; }
    std::array<double, 3> apply(const std::array<double, 3> &p) const
    {
        std::array<double, 3> o;
        for (int r = 0; r < 3; ++r)
            o[r] = ((p[0] * m_[4 * r] + p[1] * m_[4 * r + 1]) + p[2] * m_[4 * r + 2]) + m_[4 * r + 3];
        return o;
    }
    PointCloud apply(const PointCloud &cloud) const // cloud * R^T + t^T, types.hpp:110-115
    {
        std::vector<double> out(3 * cloud.size());
        for (std::size_t i = 0; i < cloud.size(); ++i) {
            const double *p = cloud.row(i);
            auto o = apply({p[0], p[1], p[2]});
            out[3 * i] = o[0];
            out[3 * i + 1] = o[1];
            out[3 * i + 2] = o[2];
        }
        return PointCloud(std::move(out));
    }
    Transformation compose(const Transformation &other) const // this applied after other
    {
        std::array<double, 16> c{};
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                double s = 0;
                for (int k = 0; k < 4; ++k) s += m_[4 * i + k] * other.m_[4 * k + j];
                c[4 * i + j] = s;
            }
        return Transformation(c);
    }
    Transformation operator*(const Transformation &other) const { return compose(other); }
    Transformation inverse() const // (R^T, -R^T t), types.hpp:128-132
    {
        std::array<double, 9> Rt;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Rt[3 * i + j] = m_[4 * j + i];
        std::array<double, 3> ti;
        for (int i = 0; i < 3; ++i) ti[i] = -(Rt[3 * i] * m_[3] + Rt[3 * i + 1] * m_[7] + Rt[3 * i + 2] * m_[11]);
        return from_rt(Rt, ti);
    }

private:
    std::array<double, 16> m_;
};

struct ICPConfig { // types.hpp:143-148
    int max_iterations = 50;
    double tolerance = 1e-6;
    double min_error = 1e-9;
    Transformation initial_transform = Transformation::identity();
};

struct ICPResult { // types.hpp:155-164
    Transformation transformation;
    bool converged = false;
    int num_iterations = 0;
    std::vector<double> error_history;
    double final_error = 0.0;
    bool success() const { return converged && final_error < 0.1; }
};

class IcpError : public std::runtime_error {
public:
    IcpError(int code, const std::string &what) : std::runtime_error(what), code_(code) {}
    int code() const { return code_; }

private:
    int code_;
};

// RAII owner of an icpmi_ctx (device buffers, stream, optional RCCL communicator).
class Context {
public:
    explicit Context(int device = 0, int normal_k = 20, int search = ICPMI_SEARCH_AUTO)
    {
        icpmi_options o;
        icpmi_options_default(&o);
        o.device = device;
        o.normal_k = normal_k;
        o.search = search;
        int rc = icpmi_create(&o, &ctx_);
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(nullptr));
    }
    ~Context() { icpmi_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    icpmi_ctx *get() const { return ctx_; }

private:
    icpmi_ctx *ctx_ = nullptr;
};

// One context per thread, created on first use (the reference's function is stateless;
// the context only caches device allocations between calls).
inline Context &default_context()
{
    thread_local Context ctx;
    return ctx;
}

// 6 x 6 row-major: the normal matrix of a registration, the information matrix of a pose-graph edge
using Matrix6 = std::array<double, 36>;

// icpmi_last_normal_matrix: the normal equations of the pass that produced final_error of the last registration `ctx`
// ran (problem k of the last *_batch call, 0 after a single one): JtJ and Jtb in the order [rotation; translation] of
// the registration's own step, sum_sq / weight = final_error^2, and the result T the pass ran at.  Throws IcpError
// where no registration ran or its last pass kept no row.
struct NormalMatrix {
    Matrix6 JtJ{};
    std::array<double, 6> Jtb{};
    double sum_sq = 0.0, weight = 0.0;
    long long pairs = 0;
    Transformation T;
};
inline NormalMatrix last_normal_matrix(Context &ctx, int k = 0)
{
    icpmi_normal_matrix nm;
    const int rc = icpmi_last_normal_matrix(ctx.get(), k, &nm);
    if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx.get()));
    NormalMatrix out;
    std::copy(nm.JtJ, nm.JtJ + 36, out.JtJ.begin());
    std::copy(nm.Jtb, nm.Jtb + 6, out.Jtb.begin());
    out.sum_sq = nm.sum_sq;
    out.weight = nm.weight;
    out.pairs = nm.pairs;
    std::array<double, 16> m;
    std::copy(nm.T, nm.T + 16, m.begin());
    out.T = Transformation(m);
    return out;
}

// icpmi_information_from_icp (host only, no device): the information of the pose-graph edge entered as rel = T, from the
// target's pose to the source's, of a registration with normal matrix JtJ at result T.  sigma: the residual noise of
// one pair in metres; the floors (0: none) are sigmas of an isotropic term that keeps a rank-deficient JtJ positive
// definite.
inline Matrix6 information_from_icp(const Matrix6 &JtJ, const Transformation &T, double sigma,
                                    double floor_rotation_sigma = 0.0, double floor_translation_sigma = 0.0)
{
    Matrix6 out;
    const int rc = icpmi_information_from_icp(JtJ.data(), T.matrix().data(), sigma, floor_rotation_sigma,
                                              floor_translation_sigma, out.data());
    if (rc != ICPMI_OK)
        throw IcpError(rc, "information_from_icp: sigma must be finite and > 0, a floor 0 or finite and > 0, JtJ and T finite");
    return out;
}

namespace detail {
inline icpmi_config to_c(const ICPConfig &c)
{
    icpmi_config k;
    icpmi_config_default(&k);
    k.max_iterations = c.max_iterations;
    k.tolerance = c.tolerance;
    k.min_error = c.min_error;
    for (int i = 0; i < 16; ++i) k.initial_transform[i] = c.initial_transform.matrix()[i];
    return k;
}
} // namespace detail

// Raw-pointer form: row-major N x 3 fp64 clouds (what PointCloud::points().data() is in
// the reference, types.hpp:17).
inline ICPResult icp_point_to_plane(Context &ctx, const double *source_xyz, std::size_t n_src,
                                    const double *target_xyz, std::size_t n_tgt,
                                    const ICPConfig &config = ICPConfig())
{
    icpmi_config k = detail::to_c(config);
    std::vector<double> hist(static_cast<std::size_t>(config.max_iterations > 0 ? config.max_iterations : 0) + 1);
    icpmi_result r;
    int rc = icpmi_align(ctx.get(), source_xyz, static_cast<int64_t>(n_src), target_xyz,
                         static_cast<int64_t>(n_tgt), &k, &r, hist.data(), static_cast<int32_t>(hist.size()));
    if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx.get()));
    ICPResult out;
    std::array<double, 16> m;
    for (int i = 0; i < 16; ++i) m[i] = r.transformation[i];
    out.transformation = Transformation(m);
    out.converged = r.converged != 0;
    out.num_iterations = r.num_iterations;
    out.final_error = r.final_error;
    hist.resize(static_cast<std::size_t>(r.history_len));
    out.error_history = std::move(hist);
    return out;
}

// Several independent registrations of one source at once (icpmi_align_batch): what the verifications of one
// LoopClosureDetector::detect() are (loop_closure.hpp:94-123).  Each result is that of icp_point_to_plane alone.
// initial_transforms: empty (config's for every target), or one per target (each verification its own start).
inline std::vector<ICPResult> icp_point_to_plane_batch(Context &ctx, const PointCloud &source,
                                                       const std::vector<const PointCloud *> &targets, const ICPConfig &config,
                                                       const std::vector<Transformation> &initial_transforms = {})
{
    const std::size_t k = targets.size();
    std::vector<ICPResult> out(k);
    if (k == 0) return out;
    if (!initial_transforms.empty() && initial_transforms.size() != k)
        throw IcpError(ICPMI_ERR_ARG, "as many initial transforms as targets, or none");
    std::vector<const double *> sp(k, source.data()), tp(k);
    std::vector<int64_t> ns(k, static_cast<int64_t>(source.size())), nt(k);
    for (std::size_t i = 0; i < k; ++i) {
        tp[i] = targets[i]->data();
        nt[i] = static_cast<int64_t>(targets[i]->size());
    }
    std::vector<icpmi_config> cfgs(k, detail::to_c(config));
    for (std::size_t i = 0; i < initial_transforms.size(); ++i)
        for (int e = 0; e < 16; ++e) cfgs[i].initial_transform[e] = initial_transforms[i].matrix()[static_cast<std::size_t>(e)];
    const std::size_t stride = static_cast<std::size_t>(config.max_iterations > 0 ? config.max_iterations : 0) + 1;
    std::vector<double> hist(k * stride);
    std::vector<icpmi_result> res(k);
    std::vector<int32_t> status(k);
    const int rc = icpmi_align_batch(ctx.get(), static_cast<int32_t>(k), sp.data(), ns.data(), tp.data(), nt.data(), cfgs.data(),
                                     res.data(), hist.data(), static_cast<int32_t>(stride), status.data());
    if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx.get()));
    for (std::size_t i = 0; i < k; ++i) {
        std::array<double, 16> m;
        for (int e = 0; e < 16; ++e) m[e] = res[i].transformation[e];
        out[i].transformation = Transformation(m);
        out[i].converged = res[i].converged != 0;
        out[i].num_iterations = res[i].num_iterations;
        out[i].final_error = res[i].final_error;
        out[i].error_history.assign(hist.begin() + static_cast<std::ptrdiff_t>(i * stride),
                                    hist.begin() + static_cast<std::ptrdiff_t>(i * stride) + res[i].history_len);
    }
    return out;
}

// ---- the correspondence-distance gate (icpmi_align_gated*; not in the reference) -----------------
// A pass sums only the rows whose nearest target is within max_distance (metres; finite, > 0), and the error is the
// RMS over those.  pairs: the rows kept by the pass that produced final_error, of `rows`.  A pass that keeps none ends
// the call unconverged with final_error = +Inf.  A gate that keeps every row gives icp_point_to_plane's bits.
struct GatedICPResult : ICPResult {
    long long pairs = 0;
    long long rows = 0;
};

namespace detail {
inline void fill(ICPResult &out, const icpmi_result &r, const double *hist)
{
    std::array<double, 16> m;
    for (int e = 0; e < 16; ++e) m[static_cast<std::size_t>(e)] = r.transformation[e];
    out.transformation = Transformation(m);
    out.converged = r.converged != 0;
    out.num_iterations = r.num_iterations;
    out.final_error = r.final_error;
    out.error_history.assign(hist, hist + r.history_len);
}
} // namespace detail

inline GatedICPResult align_gated(Context &ctx, const double *source_xyz, std::size_t n_src, const double *target_xyz,
                                  std::size_t n_tgt, double max_distance, const ICPConfig &config = ICPConfig())
{
    icpmi_config k = detail::to_c(config);
    icpmi_gate g{};
    g.max_distance = max_distance;
    icpmi_gate_info info{};
    std::vector<double> hist(static_cast<std::size_t>(config.max_iterations > 0 ? config.max_iterations : 0) + 1);
    icpmi_result r;
    const int rc = icpmi_align_gated(ctx.get(), source_xyz, static_cast<int64_t>(n_src), target_xyz, static_cast<int64_t>(n_tgt),
                                     &k, &g, &r, &info, hist.data(), static_cast<int32_t>(hist.size()));
    if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx.get()));
    GatedICPResult out;
    detail::fill(out, r, hist.data());
    out.pairs = info.pairs;
    out.rows = info.rows;
    return out;
}
inline GatedICPResult align_gated(const PointCloud &source, const PointCloud &target, double max_distance,
                                  const ICPConfig &config = ICPConfig())
{
    return align_gated(default_context(), source.data(), source.size(), target.data(), target.size(), max_distance, config);
}

// icp_point_to_plane_batch behind one gate for every problem (icpmi_align_gated_batch): each result is that of
// align_gated alone.
inline std::vector<GatedICPResult> align_gated_batch(Context &ctx, const PointCloud &source,
                                                     const std::vector<const PointCloud *> &targets, double max_distance,
                                                     const ICPConfig &config,
                                                     const std::vector<Transformation> &initial_transforms = {})
{
    const std::size_t k = targets.size();
    std::vector<GatedICPResult> out(k);
    if (k == 0) return out;
    if (!initial_transforms.empty() && initial_transforms.size() != k)
        throw IcpError(ICPMI_ERR_ARG, "as many initial transforms as targets, or none");
    std::vector<const double *> sp(k, source.data()), tp(k);
    std::vector<int64_t> ns(k, static_cast<int64_t>(source.size())), nt(k);
    for (std::size_t i = 0; i < k; ++i) {
        tp[i] = targets[i]->data();
        nt[i] = static_cast<int64_t>(targets[i]->size());
    }
    std::vector<icpmi_config> cfgs(k, detail::to_c(config));
    for (std::size_t i = 0; i < initial_transforms.size(); ++i)
        for (int e = 0; e < 16; ++e) cfgs[i].initial_transform[e] = initial_transforms[i].matrix()[static_cast<std::size_t>(e)];
    icpmi_gate g{};
    g.max_distance = max_distance;
    std::vector<icpmi_gate> gates(k, g);
    std::vector<icpmi_gate_info> infos(k);
    const std::size_t stride = static_cast<std::size_t>(config.max_iterations > 0 ? config.max_iterations : 0) + 1;
    std::vector<double> hist(k * stride);
    std::vector<icpmi_result> res(k);
    std::vector<int32_t> status(k);
    const int rc = icpmi_align_gated_batch(ctx.get(), static_cast<int32_t>(k), sp.data(), ns.data(), tp.data(), nt.data(),
                                           cfgs.data(), gates.data(), res.data(), infos.data(), hist.data(),
                                           static_cast<int32_t>(stride), status.data());
    if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx.get()));
    for (std::size_t i = 0; i < k; ++i) {
        detail::fill(out[i], res[i], hist.data() + i * stride);
        out[i].pairs = infos[i].pairs;
        out[i].rows = infos[i].rows;
    }
    return out;
}

// ---- robust row weights (icpmi_align_robust*; not in the reference) ------------------------------
// A pass weights each kept row by its point-to-plane residual b (kind ICPMI_ROBUST_HUBER: w = |b| <= scale ? 1 :
// scale / |b|; ICPMI_ROBUST_GEMAN_MCCLURE: w = (scale^2 / (scale^2 + b^2))^2), optionally behind the gate above
// (max_distance; 0: none); icpmi_align_robust in icp_mi355x.h has the contract.  final_error and the history are the
// WEIGHTED RMS sqrt(sum w b^2 / sum w), which reads lower than the plain one: a caller's thresholds on it see that
// number.  weight_sum and pairs: of the pass that produced final_error, of `rows`.
struct RobustRule {
    int kind = ICPMI_ROBUST_HUBER;
    double scale = 0.1;
    double max_distance = 0.0;
};
struct RobustICPResult : ICPResult {
    double weight_sum = 0.0;
    long long pairs = 0;
    long long rows = 0;
};

namespace detail {
inline icpmi_robust to_c(const RobustRule &rule)
{
    icpmi_robust r{};
    r.kind = rule.kind;
    r.scale = rule.scale;
    r.max_distance = rule.max_distance;
    return r;
}
} // namespace detail

inline RobustICPResult align_robust(Context &ctx, const double *source_xyz, std::size_t n_src, const double *target_xyz,
                                    std::size_t n_tgt, const RobustRule &rule, const ICPConfig &config = ICPConfig())
{
    icpmi_config k = detail::to_c(config);
    const icpmi_robust g = detail::to_c(rule);
    icpmi_robust_info info{};
    std::vector<double> hist(static_cast<std::size_t>(config.max_iterations > 0 ? config.max_iterations : 0) + 1);
    icpmi_result r;
    const int rc = icpmi_align_robust(ctx.get(), source_xyz, static_cast<int64_t>(n_src), target_xyz, static_cast<int64_t>(n_tgt),
                                      &k, &g, &r, &info, hist.data(), static_cast<int32_t>(hist.size()));
    if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx.get()));
    RobustICPResult out;
    detail::fill(out, r, hist.data());
    out.weight_sum = info.weight_sum;
    out.pairs = info.pairs;
    out.rows = info.rows;
    return out;
}
inline RobustICPResult align_robust(const PointCloud &source, const PointCloud &target, const RobustRule &rule,
                                    const ICPConfig &config = ICPConfig())
{
    return align_robust(default_context(), source.data(), source.size(), target.data(), target.size(), rule, config);
}

// icp_point_to_plane_batch under one rule for every problem (icpmi_align_robust_batch): each result is that of
// align_robust alone.
inline std::vector<RobustICPResult> align_robust_batch(Context &ctx, const PointCloud &source,
                                                       const std::vector<const PointCloud *> &targets, const RobustRule &rule,
                                                       const ICPConfig &config,
                                                       const std::vector<Transformation> &initial_transforms = {})
{
    const std::size_t k = targets.size();
    std::vector<RobustICPResult> out(k);
    if (k == 0) return out;
    if (!initial_transforms.empty() && initial_transforms.size() != k)
        throw IcpError(ICPMI_ERR_ARG, "as many initial transforms as targets, or none");
    std::vector<const double *> sp(k, source.data()), tp(k);
    std::vector<int64_t> ns(k, static_cast<int64_t>(source.size())), nt(k);
    for (std::size_t i = 0; i < k; ++i) {
        tp[i] = targets[i]->data();
        nt[i] = static_cast<int64_t>(targets[i]->size());
    }
    std::vector<icpmi_config> cfgs(k, detail::to_c(config));
    for (std::size_t i = 0; i < initial_transforms.size(); ++i)
        for (int e = 0; e < 16; ++e) cfgs[i].initial_transform[e] = initial_transforms[i].matrix()[static_cast<std::size_t>(e)];
    std::vector<icpmi_robust> rules(k, detail::to_c(rule));
    std::vector<icpmi_robust_info> infos(k);
    const std::size_t stride = static_cast<std::size_t>(config.max_iterations > 0 ? config.max_iterations : 0) + 1;
    std::vector<double> hist(k * stride);
    std::vector<icpmi_result> res(k);
    std::vector<int32_t> status(k);
    const int rc = icpmi_align_robust_batch(ctx.get(), static_cast<int32_t>(k), sp.data(), ns.data(), tp.data(), nt.data(),
                                            cfgs.data(), rules.data(), res.data(), infos.data(), hist.data(),
                                            static_cast<int32_t>(stride), status.data());
    if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx.get()));
    for (std::size_t i = 0; i < k; ++i) {
        detail::fill(out[i], res[i], hist.data() + i * stride);
        out[i].weight_sum = infos[i].weight_sum;
        out[i].pairs = infos[i].pairs;
        out[i].rows = infos[i].rows;
    }
    return out;
}

// ---- plane-to-plane (generalized) ICP (icpmi_align_gicp*; not in the reference) ---------------------
// Both clouds carry a local surface model, I - (1 - epsilon) n n^T of each row's normal, and every correspondence is
// weighted by the inverse of the two summed; optionally behind the gate above (max_distance; 0: none).  epsilon = 1 is
// point-to-point ICP.  icpmi_align_gicp in icp_mi355x.h has the contract; final_error and the history read in metres.
// pairs: the rows kept by the pass that produced final_error, of `rows`.  (No overload in the Eigen adapter, as for
// the gate: the adapter mirrors the reference's call shapes only.)
// small_form (ICPMI_GICP_FORM_SMALL): at the sizes the small-cloud kernel takes, a pass is one kernel; the result agrees
// with the general path's to rounding, not to bits.  Off: the general path at every size.
struct GicpRule {
    double epsilon = ICPMI_GICP_EPSILON_DEFAULT;
    double max_distance = 0.0;
    bool small_form = false;
};
struct GicpICPResult : ICPResult {
    long long pairs = 0;
    long long rows = 0;
};

inline GicpICPResult align_gicp(Context &ctx, const double *source_xyz, std::size_t n_src, const double *target_xyz,
                                std::size_t n_tgt, const GicpRule &rule, const ICPConfig &config = ICPConfig())
{
    icpmi_config k = detail::to_c(config);
    icpmi_gicp g{};
    g.epsilon = rule.epsilon;
    g.max_distance = rule.max_distance;
    g.reserved = rule.small_form ? ICPMI_GICP_FORM_SMALL : 0;
    icpmi_gicp_info info{};
    std::vector<double> hist(static_cast<std::size_t>(config.max_iterations > 0 ? config.max_iterations : 0) + 1);
    icpmi_result r;
    const int rc = icpmi_align_gicp(ctx.get(), source_xyz, static_cast<int64_t>(n_src), target_xyz, static_cast<int64_t>(n_tgt),
                                    &k, &g, &r, &info, hist.data(), static_cast<int32_t>(hist.size()));
    if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx.get()));
    GicpICPResult out;
    detail::fill(out, r, hist.data());
    out.pairs = info.pairs;
    out.rows = info.rows;
    return out;
}
inline GicpICPResult align_gicp(const PointCloud &source, const PointCloud &target, const GicpRule &rule = GicpRule(),
                                const ICPConfig &config = ICPConfig())
{
    return align_gicp(default_context(), source.data(), source.size(), target.data(), target.size(), rule, config);
}

// icp_point_to_plane_batch under one rule for every problem (icpmi_align_gicp_batch): each result is that of align_gicp
// alone.
inline std::vector<GicpICPResult> align_gicp_batch(Context &ctx, const PointCloud &source,
                                                   const std::vector<const PointCloud *> &targets, const GicpRule &rule,
                                                   const ICPConfig &config,
                                                   const std::vector<Transformation> &initial_transforms = {})
{
    const std::size_t k = targets.size();
    std::vector<GicpICPResult> out(k);
    if (k == 0) return out;
    if (!initial_transforms.empty() && initial_transforms.size() != k)
        throw IcpError(ICPMI_ERR_ARG, "as many initial transforms as targets, or none");
    std::vector<const double *> sp(k, source.data()), tp(k);
    std::vector<int64_t> ns(k, static_cast<int64_t>(source.size())), nt(k);
    for (std::size_t i = 0; i < k; ++i) {
        tp[i] = targets[i]->data();
        nt[i] = static_cast<int64_t>(targets[i]->size());
    }
    std::vector<icpmi_config> cfgs(k, detail::to_c(config));
    for (std::size_t i = 0; i < initial_transforms.size(); ++i)
        for (int e = 0; e < 16; ++e) cfgs[i].initial_transform[e] = initial_transforms[i].matrix()[static_cast<std::size_t>(e)];
    icpmi_gicp g{};
    g.epsilon = rule.epsilon;
    g.max_distance = rule.max_distance;
    g.reserved = rule.small_form ? ICPMI_GICP_FORM_SMALL : 0;
    std::vector<icpmi_gicp> rules(k, g);
    std::vector<icpmi_gicp_info> infos(k);
    const std::size_t stride = static_cast<std::size_t>(config.max_iterations > 0 ? config.max_iterations : 0) + 1;
    std::vector<double> hist(k * stride);
    std::vector<icpmi_result> res(k);
    std::vector<int32_t> status(k);
    const int rc = icpmi_align_gicp_batch(ctx.get(), static_cast<int32_t>(k), sp.data(), ns.data(), tp.data(), nt.data(),
                                          cfgs.data(), rules.data(), res.data(), infos.data(), hist.data(),
                                          static_cast<int32_t>(stride), status.data());
    if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx.get()));
    for (std::size_t i = 0; i < k; ++i) {
        detail::fill(out[i], res[i], hist.data() + i * stride);
        out[i].pairs = infos[i].pairs;
        out[i].rows = infos[i].rows;
    }
    return out;
}

// Same call shape as slam::icp_point_to_plane (icp.hpp:157-161).
inline ICPResult icp_point_to_plane(const PointCloud &source, const PointCloud &target,
                                    const ICPConfig &config = ICPConfig())
{
    return icp_point_to_plane(default_context(), source.data(), source.size(), target.data(),
                              target.size(), config);
}

// Same call shape as slam::voxel_downsample (src/core/file_utils.cpp:148-196); voxels come
// out sorted by key (the reference's order is std::unordered_map iteration order).
inline PointCloud voxel_downsample(Context &ctx, const PointCloud &points, double voxel_size)
{
    std::vector<double> out(3 * points.size());
    int64_t rows = 0;
    int rc = icpmi_voxel_downsample(ctx.get(), points.data(), static_cast<int64_t>(points.size()), voxel_size,
                                    out.data(), static_cast<int64_t>(points.size()), &rows);
    if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx.get()));
    out.resize(3 * static_cast<std::size_t>(rows));
    return PointCloud(std::move(out));
}
inline PointCloud voxel_downsample(const PointCloud &points, double voxel_size)
{
    return voxel_downsample(default_context(), points, voxel_size);
}

// ---- stage-level mirrors (the pieces slam::icp_point_to_plane is made of) ------------------------
// slam::KDTree (kdtree.hpp:18-186).  The device search needs no tree: the object keeps the target
// rows (as the reference's constructor copies them, kdtree.hpp:20) and searches through the C ABI.
class KDTree {
public:
    explicit KDTree(const PointCloud &points, Context *ctx = nullptr) : pts_(points.copy()), ctx_(ctx) {}
    std::size_t size() const { return pts_.size(); }
    const PointCloud &points() const { return pts_; }
    // kdtree.hpp:43-59: nearest target row and squared distance for every query row
    void nearest_batch(const PointCloud &queries, std::vector<int> &indices, std::vector<double> &distances_sq) const
    {
        indices.assign(queries.size(), -1);
        distances_sq.assign(queries.size(), 0.0);
        if (queries.empty()) return;
        Context &c = ctx_ ? *ctx_ : default_context();
        std::vector<int32_t> idx(queries.size());
        int rc = icpmi_nearest_batch(c.get(), pts_.data(), static_cast<int64_t>(pts_.size()), queries.data(),
                                     static_cast<int64_t>(queries.size()), idx.data(), distances_sq.data());
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(c.get()));
        for (std::size_t i = 0; i < idx.size(); ++i) indices[i] = idx[i];
    }
    // kdtree.hpp:28-38: (index, squared distance) of the nearest row to one point
    std::pair<int, double> nearest(const std::array<double, 3> &query) const
    {
        std::vector<int> i;
        std::vector<double> d;
        nearest_batch(PointCloud(query.data(), 1), i, d);
        return {i[0], d[0]};
    }
    // kdtree.hpp:65-78: indices of the k nearest rows to one point, closest first
    std::vector<int> k_nearest(const std::array<double, 3> &query, int k) const
    {
        std::vector<int32_t> idx(static_cast<std::size_t>(k > 0 ? k : 0), -1);
        Context &c = ctx_ ? *ctx_ : default_context();
        int rc = icpmi_k_nearest(c.get(), pts_.data(), static_cast<int64_t>(pts_.size()), query.data(), 1, k, idx.data(), nullptr);
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(c.get()));
        std::vector<int> out;
        for (int32_t j : idx)
            if (j >= 0) out.push_back(j);
        return out;
    }

private:
    PointCloud pts_;
    Context *ctx_;
};

// slam::NearestNeighborSearch (kdtree.hpp:193-221)
class NearestNeighborSearch {
public:
    explicit NearestNeighborSearch(const PointCloud &target, Context *ctx = nullptr) : tree_(target, ctx) {}
    const KDTree &tree() const { return tree_; }
    // kdtree.hpp:198-214: matched_target.row(i) = target.row(nearest(i)), distances = sqrt(d^2)
    void find_correspondences(const PointCloud &source, PointCloud &matched_target, std::vector<double> &distances) const
    {
        std::vector<int> idx;
        std::vector<double> d2;
        tree_.nearest_batch(source, idx, d2);
        std::vector<double> rows(3 * source.size());
        distances.resize(source.size());
        for (std::size_t i = 0; i < source.size(); ++i) {
            const double *q = tree_.points().row(static_cast<std::size_t>(idx[i]));
            rows[3 * i] = q[0];
            rows[3 * i + 1] = q[1];
            rows[3 * i + 2] = q[2];
            distances[i] = std::sqrt(d2[i]);
        }
        matched_target = PointCloud(std::move(rows));
    }

private:
    KDTree tree_;
};

// slam::estimate_normals (icp.hpp:23-67): unit normals of `points` from their k nearest neighbours
inline PointCloud estimate_normals(const PointCloud &points, int k = 20, Context *ctx = nullptr)
{
    Context &c = ctx ? *ctx : default_context();
    std::vector<double> out(3 * points.size());
    int rc = icpmi_estimate_normals(c.get(), points.data(), static_cast<int64_t>(points.size()), k, out.data());
    if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(c.get()));
    return PointCloud(std::move(out));
}

// slam::solve_point_to_plane (icp.hpp:89-144): one linearised step for given correspondences
inline Transformation solve_point_to_plane(const PointCloud &source, const PointCloud &target, const PointCloud &normals,
                                           Context *ctx = nullptr)
{
    if (source.size() != target.size() || source.size() != normals.size())
        throw std::invalid_argument("solve_point_to_plane: row counts differ");
    Context &c = ctx ? *ctx : default_context();
    std::array<double, 16> T{};
    int rc = icpmi_solve_point_to_plane(c.get(), source.data(), target.data(), normals.data(),
                                        static_cast<int64_t>(source.size()), T.data());
    if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(c.get()));
    return Transformation(T);
}

// ---- the caller's frame step (slam_viz/src/ros/slam_node.cpp:118-157) ---------------------------------
struct OccupancyGridConfig { // slam_node.hpp:35-40
    double resolution = 0.2;
    double height_min = 0.3;
    double height_max = 2.0;
    double max_range = 40.0;
};
struct GridCell { // slam_node.hpp:45-50
    int x, y;
    bool operator==(const GridCell &o) const { return x == o.x && y == o.y; }
};
namespace detail {
inline icpmi_grid_config to_c(const OccupancyGridConfig &g)
{
    icpmi_grid_config c;
    c.resolution = g.resolution;
    c.height_min = g.height_min;
    c.height_max = g.height_max;
    c.max_range = g.max_range;
    return c;
}
} // namespace detail

// occupied_cells_ and the functions around it (slam_node.cpp:211-226,279-297); the set lives in the
// context's device memory, sorted by (x, y).
class OccupancyGrid {
public:
    explicit OccupancyGrid(OccupancyGridConfig config = OccupancyGridConfig(), Context *ctx = nullptr)
        : config_(config), ctx_(ctx ? ctx : &default_context())
    {
    }
    // update_occupancy_grid(cloud, sensor) (slam_node.cpp:211-221) -> cells in the set afterwards
    std::size_t update(const PointCloud &world, const std::array<double, 3> &sensor)
    {
        const icpmi_grid_config g = detail::to_c(config_);
        int64_t n = 0;
        const int rc = icpmi_occupancy_update(ctx_->get(), world.data(), static_cast<int64_t>(world.size()), sensor.data(), &g, &n);
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
        return static_cast<std::size_t>(n);
    }
    void clear() { icpmi_occupancy_clear(ctx_->get()); } // slam_node.cpp:224
    std::vector<GridCell> cells() const
    {
        int64_t n = 0;
        int rc = icpmi_occupancy_cells(ctx_->get(), nullptr, 0, &n);
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
        std::vector<GridCell> out(static_cast<std::size_t>(n));
        static_assert(sizeof(GridCell) == 2 * sizeof(int32_t), "cells are read as int32 pairs");
        if (n > 0) {
            rc = icpmi_occupancy_cells(ctx_->get(), reinterpret_cast<int32_t *>(out.data()), n, &n);
            if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
        }
        return out;
    }
    const OccupancyGridConfig &config() const { return config_; }

private:
    OccupancyGridConfig config_;
    Context *ctx_;
};

// Motion compensation (deskew) of a scan in its sensor frame (icpmi_deskew; not in the reference, which takes every scan
// as a snapshot from one pose).  twist = (omega, v): the sensor's motion over one whole sweep, in the sensor frame; row i,
// measured at tau_i in [0, 1], becomes Exp((tau_i - t_ref) twist) p_i.  The defaults are icpmi_deskew_config_default's,
// except time_source: deskew() sets it from whether times are given, OdometryStream::set_deskew to Azimuth.
enum class DeskewTimeSource : int32_t { Times = ICPMI_DESKEW_TIMES, Azimuth = ICPMI_DESKEW_AZIMUTH };
struct DeskewConfig {
    std::array<double, 6> twist{{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
    double t_ref = 0.5;                        // the moment of the sweep the deskewed scan is registered as
    int direction = 1;                         // +1: the azimuth grows with time; -1: clockwise
    double azimuth_start = -3.14159265358979323846; // the azimuth at tau = 0
};

namespace detail {
inline icpmi_deskew_config to_c(const DeskewConfig &c, DeskewTimeSource source)
{
    icpmi_deskew_config k;
    icpmi_deskew_config_default(&k);
    for (std::size_t e = 0; e < 6; ++e) k.twist[e] = c.twist[e];
    k.t_ref = c.t_ref, k.direction = c.direction, k.azimuth_start = c.azimuth_start;
    k.time_source = static_cast<int32_t>(source);
    return k;
}
} // namespace detail

// icpmi_deskew_twist (host only, no device): the SE(3) log (omega, v) of a relative pose -- the twist of the next sweep
// under constant velocity, from this frame's delta.
inline std::array<double, 6> deskew_twist(const Transformation &delta)
{
    std::array<double, 6> twist{};
    const int rc = icpmi_deskew_twist(delta.matrix().data(), twist.data());
    if (rc != ICPMI_OK) throw IcpError(rc, "deskew_twist: a pose entry is not finite");
    return twist;
}

// the rows of `scan` at the times `times` (one per row, in [0, 1]) ...
inline PointCloud deskew(Context &ctx, const PointCloud &scan, const std::vector<double> &times, const DeskewConfig &config)
{
    if (times.size() != scan.size()) throw IcpError(ICPMI_ERR_ARG, "deskew: one time per row");
    const icpmi_deskew_config k = detail::to_c(config, DeskewTimeSource::Times);
    std::vector<double> out(3 * scan.size());
    const int rc = icpmi_deskew(ctx.get(), scan.data(), times.data(), static_cast<int64_t>(scan.size()), &k, out.data());
    if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx.get()));
    return PointCloud(std::move(out));
}
// ... or at times taken from the rows' azimuths (what a KITTI .bin, which carries none, gets)
inline PointCloud deskew(Context &ctx, const PointCloud &scan, const DeskewConfig &config)
{
    const icpmi_deskew_config k = detail::to_c(config, DeskewTimeSource::Azimuth);
    std::vector<double> out(3 * scan.size());
    const int rc = icpmi_deskew(ctx.get(), scan.data(), nullptr, static_cast<int64_t>(scan.size()), &k, out.data());
    if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx.get()));
    return PointCloud(std::move(out));
}

// process_frame as two calls per frame with the scans resident in device memory: push() is
// lines 122-138 (voxel filter, guards, registration against the previous filtered scan), the caller
// applies its gate and pose update (139-145), map_update() is lines 147-153 (world points of the
// scan just pushed, occupancy insert with the new pose's translation as the sensor position).
class OdometryStream {
public:
    explicit OdometryStream(Context *ctx = nullptr) : ctx_(ctx ? ctx : &default_context()) {}
    struct Step {
        ICPResult result;            // identity / converged = false unless `registered`
        bool registered = false;     // an ICP ran (source = this scan, target = the previous one)
        bool first_frame = false;    // slam_node.cpp:69-72
        bool too_few_points = false; // slam_node.cpp:125-130
        std::size_t filtered_points = 0;
    };
    Step push(const PointCloud &raw, double voxel_size, long long min_points, const ICPConfig &config = ICPConfig())
    {
        icpmi_config k = detail::to_c(config);
        std::vector<double> hist(static_cast<std::size_t>(config.max_iterations > 0 ? config.max_iterations : 0) + 1);
        icpmi_result out;
        icpmi_stream_info info;
        const int rc = icpmi_stream_push_host(ctx_->get(), raw.data(), static_cast<int64_t>(raw.size()), voxel_size, min_points, &k,
                                              &out, hist.data(), static_cast<int32_t>(hist.size()), &info);
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
        return finish(out, info, std::move(hist));
    }
    // the scan as a file (load_ply / load_bin, slam_node.cpp:121)
    Step push_file(const std::string &path, double voxel_size, long long min_points, const ICPConfig &config = ICPConfig())
    {
        icpmi_config k = detail::to_c(config);
        std::vector<double> hist(static_cast<std::size_t>(config.max_iterations > 0 ? config.max_iterations : 0) + 1);
        icpmi_result out;
        icpmi_stream_info info;
        const int rc = icpmi_stream_push_file(ctx_->get(), path.c_str(), voxel_size, min_points, &k, &out, hist.data(),
                                              static_cast<int32_t>(hist.size()), &info);
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
        return finish(out, info, std::move(hist));
    }
    // start reading the NEXT frame's file on the context's worker thread; call before pushing the current frame
    void prefetch_file(const std::string &path) { icpmi_stream_prefetch_file(ctx_->get(), path.c_str()); }
    // world = curr * R^T + t^T (:147) of the scan just pushed; with `grid`, update_occupancy_grid(world, t) (:153)
    // into the context's cell set (read it through OccupancyGrid::cells / raster on the same context)
    PointCloud map_update(const Transformation &new_pose, const OccupancyGridConfig *grid = nullptr, std::size_t *n_cells = nullptr)
    {
        int64_t nw = static_cast<int64_t>(last_filtered_), nc = 0;
        std::vector<double> world(3 * last_filtered_);
        icpmi_grid_config g;
        if (grid) g = detail::to_c(*grid);
        const int rc = icpmi_stream_map_update(ctx_->get(), new_pose.matrix().data(), grid ? &g : nullptr, world.data(), nw, &nw, &nc);
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
        if (n_cells) *n_cells = static_cast<std::size_t>(nc);
        return PointCloud(std::move(world));
    }
    // `curr` (slam_node.cpp:122) of the frame just pushed, for what the node does with it on the host (:160)
    PointCloud current_scan() const
    {
        int64_t n = static_cast<int64_t>(last_filtered_);
        std::vector<double> xyz(3 * last_filtered_);
        const int rc = icpmi_stream_current_scan(ctx_->get(), xyz.data(), n, &n);
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
        return PointCloud(std::move(xyz));
    }
    void reset() { icpmi_stream_reset(ctx_->get()); }
    // Not in the reference: every later push registers under the rule's row weights (icpmi_stream_set_robust; the
    // rule survives reset()); clear_robust() turns them off.  last_robust(): weight sum, pairs and rows of the last
    // push's registration.  final_error is then the weighted RMS, which reads lower against the caller's `> 1.0`.
    void set_robust(const RobustRule &rule)
    {
        const icpmi_robust r = detail::to_c(rule);
        const int rc = icpmi_stream_set_robust(ctx_->get(), &r);
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
    }
    void clear_robust()
    {
        const int rc = icpmi_stream_set_robust(ctx_->get(), nullptr);
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
    }
    icpmi_robust_info last_robust() const
    {
        icpmi_robust_info info{};
        const int rc = icpmi_stream_last_robust(ctx_->get(), &info);
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
        return info;
    }
    // Not in the reference: every later push() first deskews the raw scan under `config`, its times taken from the rows'
    // azimuths (icpmi_stream_set_deskew; the setting survives reset()); clear_deskew() turns that off.  Set the twist
    // before each push -- deskew_twist(the last delta) is the constant-velocity choice.  push_file and prefetch_file
    // are refused while it is set.
    void set_deskew(const DeskewConfig &config)
    {
        const icpmi_deskew_config k = detail::to_c(config, DeskewTimeSource::Azimuth);
        const int rc = icpmi_stream_set_deskew(ctx_->get(), &k);
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
    }
    void clear_deskew()
    {
        const int rc = icpmi_stream_set_deskew(ctx_->get(), nullptr);
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
    }

private:
    Step finish(const icpmi_result &out, const icpmi_stream_info &info, std::vector<double> hist)
    {
        Step step;
        step.filtered_points = last_filtered_ = static_cast<std::size_t>(info.n_filtered);
        step.first_frame = info.status == ICPMI_STREAM_FIRST_FRAME;
        step.too_few_points = info.status == ICPMI_STREAM_TOO_FEW_POINTS;
        step.registered = info.status == ICPMI_STREAM_REGISTERED;
        if (step.registered) {
            std::array<double, 16> m;
            for (int i = 0; i < 16; ++i) m[i] = out.transformation[i];
            step.result.transformation = Transformation(m);
            step.result.converged = out.converged != 0;
            step.result.num_iterations = out.num_iterations;
            step.result.final_error = out.final_error;
            hist.resize(static_cast<std::size_t>(out.history_len));
            step.result.error_history = std::move(hist);
        }
        return step;
    }
    Context *ctx_;
    std::size_t last_filtered_ = 0;
};

// ---- loop closure: Scan Context candidates + ICP verification (core/scan_context.hpp, core/loop_closure.hpp) ----
// slam::ScanContext: the 20 x 60 max-height descriptor and its column-shift cosine distance.
class ScanContext {
public:
    static constexpr int kRings = ICPMI_SC_RINGS, kSectors = ICPMI_SC_SECTORS;
    ScanContext() : d_(static_cast<std::size_t>(kRings) * kSectors, 0.0) {}
    static ScanContext compute(const PointCloud &cloud, Context *ctx = nullptr) // scan_context.hpp:44-82
    {
        Context &c = ctx ? *ctx : default_context();
        ScanContext sc;
        const int rc = icpmi_scan_context(c.get(), cloud.data(), static_cast<int64_t>(cloud.size()), sc.d_.data());
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(c.get()));
        return sc;
    }
    double distance(const ScanContext &other, Context *ctx = nullptr) const // scan_context.hpp:90-101
    {
        Context &c = ctx ? *ctx : default_context();
        double d = 0.0;
        const int rc = icpmi_scan_context_distances(c.get(), d_.data(), other.d_.data(), 1, &d);
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(c.get()));
        return d;
    }
    const std::vector<double> &descriptor() const { return d_; } // row-major [ring][sector]

private:
    std::vector<double> d_;
};

struct LoopClosureConfig { // loop_closure.hpp:14-19
    int frame_gap = 50;
    double sc_distance_threshold = 0.25;
    double icp_fitness_threshold = 0.3;
    int max_candidates = 3;
    // Not in the reference: keep the column shift that attained each candidate's distance and start its verification
    // from Rz(shift * 6 deg) (icpmi_sc_shift_transform) instead of from the identity, so that a place revisited with
    // another heading closes too.  Off: the reference's behaviour.
    bool yaw_guess = false;
    // Not in the reference: > 0 runs the verifications behind that correspondence-distance gate (align_gated; metres),
    // so that a place revisited a lane aside, whose scans overlap only partly, closes too; icp_fitness is then the RMS
    // over the kept rows.  2 m suits 0.5 m voxel-filtered street scans; a tight gate (1 m) can make the kept set
    // alternate between passes until the iterations run out.  0: the reference's behaviour.
    double max_correspondence_distance = 0.0;
    // Not in the reference: a kind (ICPMI_ROBUST_*) runs the verifications under those row weights (align_robust), behind
    // the gate above if that is set too; icp_fitness is then the weighted RMS, which reads lower than the plain one
    // against icp_fitness_threshold.  0: the reference's behaviour.
    int robust_kind = 0;
    double robust_scale = 0.0;
    // Not in the reference: 0 < epsilon <= 1 runs the verifications as plane-to-plane registrations in their small form
    // (align_gicp with GicpRule::small_form), behind the gate above if that is set too; `pairs` is then reported, gate or
    // not.  Not together with robust_kind (ICPMI_ERR_ARG).  0: the reference's behaviour.
    double gicp_epsilon = 0.0;
    // Not in the reference: > 0 attaches to each result the information matrix of its edge, information_from_icp on that
    // verification's own normal matrix with this sigma and these floors -- what PoseGraph::addLoopClosureInformation takes.
    double information_sigma = 0.0;
    double information_floor_rotation = 0.0, information_floor_translation = 0.0;
};
struct LoopClosureResult { // loop_closure.hpp:25-31
    int query_frame = 0, match_frame = 0;
    Transformation transform;
    double scan_context_distance = 0.0, icp_fitness = 0.0;
    int sector_shift = -1; // the shift the verification started from (-1: yaw_guess off)
    long long pairs = -1;  // the rows the verification's last pass kept (-1: neither a correspondence-distance gate nor gicp_epsilon)
    double weight_sum = -1.0; // that pass's weight sum (-1: no robust weights)
    bool has_information = false; // information_sigma was set: `information` is the edge's 6 x 6 information matrix
    Matrix6 information{};
};

// icpmi_sc_shift_transform: the start of a verification whose candidate matched at column shift `shift` (0..59).
inline Transformation sc_shift_transform(int shift)
{
    std::array<double, 16> m;
    const int rc = icpmi_sc_shift_transform(shift, m.data());
    if (rc != ICPMI_OK) throw IcpError(rc, "shift outside 0..59");
    return Transformation(m);
}

// slam::LoopClosureDetector (loop_closure.hpp:41-148): keeps every frame's cloud and descriptor, and
// detect() looks for closures of the most recently added frame -- the distances of its descriptor to the
// whole history in ONE device call, the candidate filter and the sort on the host as in the reference,
// up to max_candidates ICP verifications (30 iterations, tolerance 1e-6, :102-109) through the C ABI.
class LoopClosureDetector {
public:
    explicit LoopClosureDetector(LoopClosureConfig config = LoopClosureConfig(), Context *ctx = nullptr)
        : config_(config), ctx_(ctx ? ctx : &default_context())
    {
    }
    void addFrame(const PointCloud &cloud, int frame_idx) // loop_closure.hpp:53-60
    {
        const ScanContext sc = ScanContext::compute(cloud, ctx_);
        descriptors_.insert(descriptors_.end(), sc.descriptor().begin(), sc.descriptor().end());
        clouds_.push_back(cloud.copy());
        frame_indices_.push_back(frame_idx);
    }
    std::size_t size() const { return frame_indices_.size(); }
    void clear()
    {
        descriptors_.clear();
        clouds_.clear();
        frame_indices_.clear();
    }
    std::vector<LoopClosureResult> detect() // loop_closure.hpp:66-126
    {
        std::vector<LoopClosureResult> results;
        if (frame_indices_.size() < 2) return results; // :69
        constexpr std::size_t kDesc = static_cast<std::size_t>(ScanContext::kRings) * ScanContext::kSectors;
        const std::size_t q = frame_indices_.size() - 1;
        std::vector<double> dist(q);
        std::vector<int32_t> shift(config_.yaw_guess ? q : 0);
        const int rc = config_.yaw_guess
                           ? icpmi_scan_context_distances_shift(ctx_->get(), descriptors_.data() + q * kDesc, descriptors_.data(),
                                                                static_cast<int64_t>(q), dist.data(), shift.data())
                           : icpmi_scan_context_distances(ctx_->get(), descriptors_.data() + q * kDesc, descriptors_.data(),
                                                          static_cast<int64_t>(q), dist.data()); // :84 for every i
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
        std::vector<std::pair<double, int>> candidates;
        for (std::size_t i = 0; i < q; ++i) {
            if (frame_indices_[q] - frame_indices_[i] < config_.frame_gap) continue;                       // :80-82
            if (dist[i] < config_.sc_distance_threshold) candidates.emplace_back(dist[i], static_cast<int>(i)); // :86-89
        }
        std::sort(candidates.begin(), candidates.end()); // :93
        // The reference verifies the candidates one after the other until max_candidates are ACCEPTED (:96-123).
        // The registrations are independent: the next (max_candidates - accepted) of them, all of which the
        // sequential loop would reach, run side by side (icpmi_align_batch); outcomes in the reference's order.
        int verified = 0;
        std::size_t pos = 0;
        ICPConfig icp;                                     // :102-105
        icp.max_iterations = 30;
        icp.tolerance = 1e-6;
        while (pos < candidates.size() && verified < config_.max_candidates) { // :97
            const std::size_t take = std::min<std::size_t>(candidates.size() - pos,
                                                           std::min<std::size_t>(static_cast<std::size_t>(config_.max_candidates - verified), ICPMI_MAX_BATCH));
            std::vector<const PointCloud *> tg;
            std::vector<Transformation> starts; // (the shift rides along: it never entered the order)
            for (std::size_t i = 0; i < take; ++i) {
                const std::size_t c = static_cast<std::size_t>(candidates[pos + i].second);
                tg.push_back(&clouds_[c]);
                if (config_.yaw_guess) starts.push_back(sc_shift_transform(shift[c]));
            }
            const bool gated = config_.max_correspondence_distance > 0.0;
            std::vector<ICPResult> rs; // :109
            std::vector<long long> kept(take, -1);
            std::vector<double> weight(take, -1.0);
            if (config_.gicp_epsilon != 0.0) {
                if (config_.robust_kind != 0) throw IcpError(ICPMI_ERR_ARG, "gicp_epsilon and robust_kind exclude each other");
                GicpRule rule;
                rule.epsilon = config_.gicp_epsilon;
                rule.max_distance = gated ? config_.max_correspondence_distance : 0.0;
                rule.small_form = true;
                const std::vector<GicpICPResult> gs = align_gicp_batch(*ctx_, clouds_[q], tg, rule, icp, starts);
                for (std::size_t i = 0; i < take; ++i) {
                    rs.push_back(gs[i]);
                    kept[i] = gs[i].pairs;
                }
            } else if (config_.robust_kind != 0) {
                RobustRule rule;
                rule.kind = config_.robust_kind;
                rule.scale = config_.robust_scale;
                rule.max_distance = gated ? config_.max_correspondence_distance : 0.0;
                const std::vector<RobustICPResult> gs = align_robust_batch(*ctx_, clouds_[q], tg, rule, icp, starts);
                for (std::size_t i = 0; i < take; ++i) {
                    rs.push_back(gs[i]);
                    if (gated) kept[i] = gs[i].pairs;
                    weight[i] = gs[i].weight_sum;
                }
            } else if (gated) {
                const std::vector<GatedICPResult> gs = align_gated_batch(*ctx_, clouds_[q], tg, config_.max_correspondence_distance, icp, starts);
                for (std::size_t i = 0; i < take; ++i) {
                    rs.push_back(gs[i]);
                    kept[i] = gs[i].pairs;
                }
            } else {
                rs = icp_point_to_plane_batch(*ctx_, clouds_[q], tg, icp, starts);
            }
            for (std::size_t i = 0; i < take; ++i) {
                const ICPResult &r = rs[i];
                const auto &cand = candidates[pos + i];
                if (r.converged && r.final_error < config_.icp_fitness_threshold) {              // :112
                    LoopClosureResult out;
                    out.query_frame = frame_indices_[q];
                    out.match_frame = frame_indices_[cand.second];
                    out.transform = r.transformation;
                    out.scan_context_distance = cand.first;
                    out.icp_fitness = r.final_error;
                    if (config_.yaw_guess) out.sector_shift = shift[static_cast<std::size_t>(cand.second)];
                    out.pairs = kept[i];
                    out.weight_sum = weight[i];
                    if (config_.information_sigma > 0.0) { // problem i of the batch just run
                        const NormalMatrix nm = last_normal_matrix(*ctx_, static_cast<int>(i));
                        out.information = information_from_icp(nm.JtJ, nm.T, config_.information_sigma,
                                                               config_.information_floor_rotation,
                                                               config_.information_floor_translation);
                        out.has_information = true;
                    }
                    results.push_back(out);
                    ++verified;
                }
            }
            pos += take;
        }
        return results;
    }
    const LoopClosureConfig &config() const { return config_; }

private:
    LoopClosureConfig config_;
    Context *ctx_;
    std::vector<double> descriptors_; // 1200 per frame, frame-major
    std::vector<PointCloud> clouds_;
    std::vector<int> frame_indices_;
};

// `ICP(config).align(source, target)`: the facade BASELINE.json's north_star names.
class ICP {
public:
    explicit ICP(ICPConfig config = ICPConfig()) : config_(std::move(config)) {}
    ICPResult align(const PointCloud &source, const PointCloud &target) const
    {
        return icp_point_to_plane(source, target, config_);
    }
    ICPConfig &config() { return config_; }

private:
    ICPConfig config_;
};

// slam::PoseGraphConfig (pose_graph.hpp:22-40)
struct PoseGraphConfig {
    double odom_rotation_sigma = 0.01;
    double odom_translation_sigma = 0.05;
    double prior_rotation_sigma = 0.001;
    double prior_translation_sigma = 0.001;
    double loop_rotation_sigma = 0.005;
    double loop_translation_sigma = 0.025;
    int max_iterations = 100;
    double relative_error_tol = 1e-5;
    double absolute_error_tol = 1e-5;
};

// slam::PoseGraph (pose_graph.hpp:49-147) on icpmi_pose_graph: the factors and estimates live on the device of the
// context it was made with, and optimize() runs Levenberg-Marquardt there.  Non-copyable, movable.  Where the
// reference throws (addOdometryFactor from a pose with no estimate, getPose of a missing index) this throws IcpError;
// optimize() returns false where the reference's catch does.
class PoseGraph {
public:
    explicit PoseGraph(const PoseGraphConfig &config = PoseGraphConfig(), Context *ctx = nullptr)
        : ctx_(ctx ? ctx : &default_context())
    {
        icpmi_pose_graph_config c;
        icpmi_pose_graph_config_default(&c);
        c.odom_rotation_sigma = config.odom_rotation_sigma;
        c.odom_translation_sigma = config.odom_translation_sigma;
        c.prior_rotation_sigma = config.prior_rotation_sigma;
        c.prior_translation_sigma = config.prior_translation_sigma;
        c.loop_rotation_sigma = config.loop_rotation_sigma;
        c.loop_translation_sigma = config.loop_translation_sigma;
        c.max_iterations = config.max_iterations;
        c.relative_error_tol = config.relative_error_tol;
        c.absolute_error_tol = config.absolute_error_tol;
        check(icpmi_pose_graph_create(ctx_->get(), &c, &g_));
    }
    ~PoseGraph() { icpmi_pose_graph_destroy(g_); }
    PoseGraph(const PoseGraph &) = delete;
    PoseGraph &operator=(const PoseGraph &) = delete;
    PoseGraph(PoseGraph &&o) noexcept : ctx_(o.ctx_), g_(o.g_) { o.g_ = nullptr; }
    PoseGraph &operator=(PoseGraph &&o) noexcept
    {
        if (this != &o) {
            icpmi_pose_graph_destroy(g_);
            ctx_ = o.ctx_;
            g_ = o.g_;
            o.g_ = nullptr;
        }
        return *this;
    }

    void addPrior(std::size_t index, const Transformation &pose) // pose_graph.cpp:58-79
    {
        check(icpmi_pose_graph_add_prior(g_, static_cast<int64_t>(index), pose.matrix().data()));
    }
    void addOdometryFactor(std::size_t from_idx, std::size_t to_idx, const Transformation &relative_transform,
                           double fitness_score = 0.0) // :81-116
    {
        check(icpmi_pose_graph_add_odometry(g_, static_cast<int64_t>(from_idx), static_cast<int64_t>(to_idx),
                                            relative_transform.matrix().data(), fitness_score));
    }
    void addLoopClosure(std::size_t from_idx, std::size_t to_idx, const Transformation &relative_transform) // :118-141
    {
        check(icpmi_pose_graph_add_loop_closure(g_, static_cast<int64_t>(from_idx), static_cast<int64_t>(to_idx),
                                                relative_transform.matrix().data()));
    }
    bool optimize() // :147-171
    {
        icpmi_pose_graph_info info;
        const int rc = icpmi_pose_graph_optimize(g_, &info, nullptr, 0);
        if (rc == ICPMI_ERR_ARG) return false;   // a factor on a pose with no estimate: the reference's catch
        check(rc);
        return info.optimized != 0;
    }
    Transformation getPose(std::size_t index) const // :177-186
    {
        std::array<double, 16> m;
        check(icpmi_pose_graph_pose(g_, static_cast<int64_t>(index), m.data()));
        return Transformation(m);
    }
    std::vector<Transformation> getAllPoses() const // :188-200
    {
        int64_t n = 0;
        check(icpmi_pose_graph_poses(g_, nullptr, 0, &n, nullptr));
        std::vector<double> buf(16 * static_cast<std::size_t>(n));
        if (n) check(icpmi_pose_graph_poses(g_, buf.data(), n, &n, nullptr));
        std::vector<Transformation> out;
        out.reserve(static_cast<std::size_t>(n));
        for (int64_t i = 0; i < n; ++i) {
            std::array<double, 16> m;
            std::copy(buf.begin() + 16 * i, buf.begin() + 16 * (i + 1), m.begin());
            out.emplace_back(m);
        }
        return out;
    }
    // The same two factors weighted by a full 6 x 6 information matrix in the factor's tangent order (omega, v) instead
    // of the config's sigmas (icpmi_pose_graph_add_*_information; not in the reference).  A matrix that is not finite,
    // symmetric and positive definite throws IcpError(ICPMI_ERR_ARG) and changes nothing.
    void addOdometryInformation(std::size_t from_idx, std::size_t to_idx, const Transformation &relative_transform,
                                const Matrix6 &information)
    {
        check(icpmi_pose_graph_add_odometry_information(g_, static_cast<int64_t>(from_idx), static_cast<int64_t>(to_idx),
                                                        relative_transform.matrix().data(), information.data()));
    }
    void addLoopClosureInformation(std::size_t from_idx, std::size_t to_idx, const Transformation &relative_transform,
                                   const Matrix6 &information)
    {
        check(icpmi_pose_graph_add_loop_closure_information(g_, static_cast<int64_t>(from_idx), static_cast<int64_t>(to_idx),
                                                            relative_transform.matrix().data(), information.data()));
    }
    // A robust loss on the loop-closure edges (icpmi_pose_graph_set_loop_loss): kind ICPMI_PG_LOSS_*, scale in sigmas.
    // Not in the reference; off by default.
    void setLoopLoss(int kind, double scale = 0.0) { check(icpmi_pose_graph_set_loop_loss(g_, kind, scale)); }
    std::pair<int, double> loopLoss() const
    {
        int32_t kind = 0;
        double scale = 0.0;
        check(icpmi_pose_graph_loop_loss(g_, &kind, &scale));
        return {static_cast<int>(kind), scale};
    }
    // (weights, distances) of the loop closures at the optimised values, in addLoopClosure order; throws unless the
    // optimised state of the last optimize() holds
    std::pair<std::vector<double>, std::vector<double>> loopWeights() const
    {
        int64_t n = counts().second;
        std::vector<double> w(static_cast<std::size_t>(n)), d(static_cast<std::size_t>(n));
        check(icpmi_pose_graph_loop_weights(g_, w.data(), d.data(), n, &n));
        return {w, d};
    }
    // Covariances of the optimised poses (icpmi_pose_graph_marginals and its two companions; GTSAM's
    // Marginals::marginalCovariance / jointMarginalCovariance, not in the reference): blocks of H^-1 in the tangent order
    // (omega, v).  All four throw unless the optimised state of the last optimize() holds.
    Matrix6 marginalCovariance(std::size_t index) const
    {
        const int64_t idx = static_cast<int64_t>(index);
        Matrix6 out;
        check(icpmi_pose_graph_marginals(g_, &idx, 1, out.data()));
        return out;
    }
    // 6q x 6q, row-major: block (a, b) belongs to indices[a] and indices[b]; the indices must be distinct
    std::vector<double> jointMarginalCovariance(const std::vector<std::size_t> &indices) const
    {
        std::vector<int64_t> idx(indices.begin(), indices.end());
        std::vector<double> out(36 * idx.size() * idx.size());
        check(icpmi_pose_graph_marginals(g_, idx.data(), static_cast<int32_t>(idx.size()), out.data()));
        return out;
    }
    // first-order covariance of the tangent of X_i^-1 X_j
    Matrix6 relativeCovariance(std::size_t i, std::size_t j) const
    {
        Matrix6 out;
        check(icpmi_pose_graph_relative_covariance(g_, static_cast<int64_t>(i), static_cast<int64_t>(j), out.data()));
        return out;
    }
    // d^2 of a proposed edge i -> j against the graph, chi-squared with 6 degrees of freedom for a true closure;
    // edge_covariance is the edge's own noise
    double closureDistance(std::size_t i, std::size_t j, const Transformation &relative_transform,
                           const Matrix6 &edge_covariance) const
    {
        double d2 = 0.0;
        check(icpmi_pose_graph_closure_distance(g_, static_cast<int64_t>(i), static_cast<int64_t>(j),
                                                relative_transform.matrix().data(), edge_covariance.data(), &d2));
        return d2;
    }
    std::size_t size() const { return static_cast<std::size_t>(counts().first); }
    std::size_t loopClosureCount() const { return static_cast<std::size_t>(counts().second); }
    double getFinalError() const { return last().final_error; }
    int getIterations() const { return last().iterations; }
    icpmi_pose_graph *get() const { return g_; }

private:
    void check(int rc) const
    {
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
    }
    std::pair<int64_t, int64_t> counts() const
    {
        int64_t n = 0, l = 0;
        check(icpmi_pose_graph_size(g_, &n, &l, nullptr));
        return {n, l};
    }
    icpmi_pose_graph_info last() const
    {
        icpmi_pose_graph_info info;
        check(icpmi_pose_graph_size(g_, nullptr, nullptr, &info));
        return info;
    }
    Context *ctx_;
    icpmi_pose_graph *g_ = nullptr;
};

// What GlobalMap::raycast returns (icpmi_map_raster): nav_msgs/OccupancyGrid's layout, cell (x, y) at
// data[(y - min_y) * width + (x - min_x)]: 100 occupied, 0 free, -1 unknown.
struct OccupancyRaster {
    int32_t min_x = 0, min_y = 0, width = 0, height = 0;
    double resolution = 0.0;
    std::vector<int8_t> data;
};

// What GlobalMap::raycast_counts returns (icpmi_map_counts): three arrays in OccupancyRaster's layout.  hits and
// misses count the used frames that saw the cell occupied and that saw through it; probability is -1 for a cell no
// frame observed and else 100 hits / (hits + misses) rounded half up, what nav_msgs/OccupancyGrid's data carries.
struct OccupancyCounts {
    int32_t min_x = 0, min_y = 0, width = 0, height = 0;
    double resolution = 0.0;
    int64_t n_observed = 0, n_hit_cells = 0;
    int32_t max_hits = 0, max_misses = 0, frames_used = 0;
    std::vector<uint16_t> hits, misses;
    std::vector<int8_t> probability;
};

// What GlobalMap::live_update returns (icpmi_live_info, less the counts' info, which live_counts carries): the frames
// the call cast, whether remembered frames were discarded and cast again, whether the plane was reallocated and
// copied, and the plane's box in cells.
struct LiveUpdate {
    int64_t frames_cast = 0;
    bool rebuilt = false, moved = false;
    int32_t plane_x0 = 0, plane_y0 = 0, plane_w = 0, plane_h = 0;
};

// Ground segmentation of a scan in its sensor frame (icpmi_ground_segment; not in the reference, which names it as
// future work, README.md:304).  The defaults are icpmi_ground_config_default's.
struct GroundConfig {
    int n_rings = 80, n_sectors = 180;
    double min_range = 0.5, max_range = 80.5;
    double sensor_height = 1.73; // the prior: the ground lies this far below the sensor
    double max_slope = 0.15, step_tol = 0.1;
    double height_tol = 0.2;
    double clear_min = 0.3, clear_max = 2.0; // the clearance band of an obstacle, over the ground
};

enum class GroundLabel : uint8_t { Obstacle = ICPMI_GROUND_OBSTACLE, Ground = ICPMI_GROUND_GROUND, Ignored = ICPMI_GROUND_IGNORED };

// What ground_segment returns: a label per row, the row's height over its bin's ground (NaN for a row that entered no
// bin), the ground height per bin (n_rings x n_sectors, ring-major) and the counts.
struct GroundSegmentation {
    std::vector<uint8_t> labels;
    std::vector<double> height, ground_z;
    int64_t n_ground = 0, n_obstacle = 0, n_ignored = 0, bins_accepted = 0;
};

namespace detail {
inline icpmi_ground_config to_c(const GroundConfig &c)
{
    icpmi_ground_config k;
    k.n_rings = c.n_rings, k.n_sectors = c.n_sectors;
    k.min_range = c.min_range, k.max_range = c.max_range, k.sensor_height = c.sensor_height;
    k.max_slope = c.max_slope, k.step_tol = c.step_tol, k.height_tol = c.height_tol;
    k.clear_min = c.clear_min, k.clear_max = c.clear_max;
    return k;
}
} // namespace detail

inline GroundSegmentation ground_segment(Context &ctx, const PointCloud &scan, const GroundConfig &config = GroundConfig())
{
    const icpmi_ground_config k = detail::to_c(config);
    GroundSegmentation out;
    out.labels.resize(scan.size());
    out.height.resize(scan.size());
    out.ground_z.resize(static_cast<std::size_t>(std::max(k.n_rings, 0)) * static_cast<std::size_t>(std::max(k.n_sectors, 0)));
    icpmi_ground_info info{};
    const int rc = icpmi_ground_segment(ctx.get(), scan.data(), static_cast<int64_t>(scan.size()), &k, out.labels.data(),
                                        out.height.data(), out.ground_z.data(), &info);
    if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx.get()));
    out.n_ground = info.n_ground, out.n_obstacle = info.n_obstacle, out.n_ignored = info.n_ignored;
    out.bins_accepted = info.bins_accepted;
    return out;
}
inline GroundSegmentation ground_segment(const PointCloud &scan, const GroundConfig &config = GroundConfig())
{
    return ground_segment(default_context(), scan, config);
}

// The rule of the static map (icpmi_static_rule; not in the reference): a voting row is dropped if its cell was
// observed by at least min_observations frames and its occupancy probability is below min_probability (0: nothing).
struct StaticRule {
    int32_t min_probability = ICPMI_STATIC_MIN_PROBABILITY_DEFAULT;
    int32_t min_observations = ICPMI_STATIC_MIN_OBSERVATIONS_DEFAULT;
};

// What GlobalMap::world_static and finish_static report (icpmi_static_info): over the used frames, their rows, those
// that vote, those dropped and rows - dropped; and the live update at the head of the call.
struct StaticInfo {
    int64_t rows = 0, voting = 0, dropped = 0, kept = 0;
    LiveUpdate live;
};

// The node's kept scans (downsampled_clouds_, slam_node.cpp:71,123) in device memory, and what it builds from them
// with the optimised poses: rebuild_recent_clouds (:187-194), build_final_global_map (:196-209) with
// rebuild_occupancy_grid (:223-229), and the map publish_global_map sends once complete (:235-238).  finish() rebuilds
// the cell set of the context, which OccupancyGrid::cells() on the same context reads.
class GlobalMap {
public:
    static constexpr std::size_t kMaxRecentClouds = 20; // slam_node.hpp:169

    explicit GlobalMap(Context *ctx = nullptr) : ctx_(ctx ? ctx : &default_context()) { check(icpmi_map_create(ctx_->get(), &m_)); }
    ~GlobalMap() { icpmi_map_destroy(m_); }
    GlobalMap(const GlobalMap &) = delete;
    GlobalMap &operator=(const GlobalMap &) = delete;
    GlobalMap(GlobalMap &&o) noexcept : ctx_(o.ctx_), m_(o.m_), rows_(std::move(o.rows_)) { o.m_ = nullptr; }
    GlobalMap &operator=(GlobalMap &&o) noexcept
    {
        if (this != &o) {
            icpmi_map_destroy(m_);
            ctx_ = o.ctx_;
            m_ = o.m_;
            rows_ = std::move(o.rows_);
            o.m_ = nullptr;
        }
        return *this;
    }

    // downsampled_clouds_.push_back(curr) (:71, :123)
    void add_frame(const PointCloud &cloud)
    {
        check(icpmi_map_add_frame(m_, cloud.data(), static_cast<int64_t>(cloud.size())));
        rows_.push_back(cloud.size());
    }
    // the same for the scan an OdometryStream on this context pushed last, without a trip through the host
    void add_stream_frame()
    {
        const int64_t before = points();
        check(icpmi_map_add_stream_frame(m_));
        rows_.push_back(static_cast<std::size_t>(points() - before));
    }
    std::size_t frames() const { return rows_.size(); }

    // rebuild_recent_clouds (:187-194): one world cloud per frame of the last kMaxRecentClouds
    std::vector<PointCloud> recent_clouds(const std::vector<Transformation> &poses) const
    {
        const std::size_t first = rows_.size() > kMaxRecentClouds ? rows_.size() - kMaxRecentClouds : 0;
        const std::vector<double> w = world(poses, first);
        std::vector<PointCloud> out;
        std::size_t at = 0;
        for (std::size_t i = first; i < rows_.size() && i < poses.size(); ++i) {
            out.emplace_back(w.data() + 3 * at, rows_[i]);
            at += rows_[i];
        }
        return out;
    }
    // build_final_global_map (:196-209): global_map_points_
    PointCloud global_map(const std::vector<Transformation> &poses) const { return PointCloud(world(poses, 0)); }
    // rebuild_occupancy_grid (:223-229) into the context's cell set, and voxel_downsample(global map, voxel_size)
    // (:235-238) of a global map that never leaves the device
    PointCloud finish(const std::vector<Transformation> &poses, const OccupancyGridConfig &grid, double voxel_size)
    {
        const std::vector<double> P = flatten(poses);
        const icpmi_grid_config g = detail::to_c(grid);
        std::size_t rows = 0;
        for (std::size_t i = 0; i < rows_.size() && i < poses.size(); ++i) rows += rows_[i];
        std::vector<double> out(3 * std::max<std::size_t>(rows, 1));
        int64_t n = 0;
        check(icpmi_map_finish(m_, P.data(), static_cast<int64_t>(poses.size()), &g, voxel_size, out.data(),
                               static_cast<int64_t>(rows), &n, nullptr));
        out.resize(3 * static_cast<std::size_t>(n));
        return PointCloud(std::move(out));
    }
    // The kept scans ray-cast into a free / occupied / unknown raster (icpmi_map_raycast), where the reference's
    // cells_to_occupancy_grid_msg (:279-297) publishes everything but the hit cells as free.  The context's cell set
    // is not touched.
    OccupancyRaster raycast(const std::vector<Transformation> &poses, const OccupancyGridConfig &grid)
    {
        const std::vector<double> P = flatten(poses);
        const icpmi_grid_config g = detail::to_c(grid);
        icpmi_raster_info info;
        check(icpmi_map_raycast(m_, P.data(), static_cast<int64_t>(poses.size()), &g, &info));
        OccupancyRaster out;
        out.min_x = info.min_x, out.min_y = info.min_y, out.width = info.width, out.height = info.height;
        out.resolution = info.resolution;
        out.data.resize(static_cast<std::size_t>(info.width) * static_cast<std::size_t>(info.height));
        if (!out.data.empty()) check(icpmi_map_raster(m_, out.data.data(), static_cast<int64_t>(out.data.size()), nullptr));
        return out;
    }
    // The same rays counted per cell (icpmi_map_raycast_counts): a used frame adds 1 to the hits of each of its
    // distinct hit cells and 1 to the misses of every other cell its rays carve.  Neither the context's cell set nor
    // the last raycast's raster is touched.
    OccupancyCounts raycast_counts(const std::vector<Transformation> &poses, const OccupancyGridConfig &grid)
    {
        const std::vector<double> P = flatten(poses);
        const icpmi_grid_config g = detail::to_c(grid);
        icpmi_counts_info info;
        check(icpmi_map_raycast_counts(m_, P.data(), static_cast<int64_t>(poses.size()), &g, &info));
        OccupancyCounts out;
        out.min_x = info.min_x, out.min_y = info.min_y, out.width = info.width, out.height = info.height;
        out.resolution = info.resolution;
        out.n_observed = info.n_observed, out.n_hit_cells = info.n_hit_cells;
        out.max_hits = info.max_hits, out.max_misses = info.max_misses, out.frames_used = info.frames_used;
        const std::size_t cells = static_cast<std::size_t>(info.width) * static_cast<std::size_t>(info.height);
        out.hits.resize(cells), out.misses.resize(cells), out.probability.resize(cells);
        if (cells)
            check(icpmi_map_counts(m_, out.hits.data(), out.misses.data(), out.probability.data(), static_cast<int64_t>(cells),
                                   nullptr));
        return out;
    }
    // The counts kept while the node drives (icpmi_map_live_update): afterwards live_counts() is byte for byte what
    // raycast_counts(poses, grid) would return, but only the frames not cast yet are cast, unless a pose already cast
    // or the grid has changed.  Where update_occupancy_grid stands in process_frame (:152), and after
    // run_pose_graph_optimization has replaced the poses (:177-185).  counts(), raster and cell set are not touched.
    LiveUpdate live_update(const std::vector<Transformation> &poses, const OccupancyGridConfig &grid)
    {
        const std::vector<double> P = flatten(poses);
        const icpmi_grid_config g = detail::to_c(grid);
        icpmi_live_info info;
        check(icpmi_map_live_update(m_, P.data(), static_cast<int64_t>(poses.size()), &g, &info));
        LiveUpdate out;
        out.frames_cast = info.frames_cast;
        out.rebuilt = info.rebuilt != 0, out.moved = info.moved != 0;
        out.plane_x0 = info.plane_x0, out.plane_y0 = info.plane_y0, out.plane_w = info.plane_w, out.plane_h = info.plane_h;
        return out;
    }
    // the live counts of the last successful live_update (icpmi_map_live_counts): 0 x 0 before the first
    OccupancyCounts live_counts()
    {
        icpmi_live_info live;
        check(icpmi_map_live_counts(m_, nullptr, nullptr, nullptr, 0, &live));
        const icpmi_counts_info &info = live.counts;
        OccupancyCounts out;
        out.min_x = info.min_x, out.min_y = info.min_y, out.width = info.width, out.height = info.height;
        out.resolution = info.resolution;
        out.n_observed = info.n_observed, out.n_hit_cells = info.n_hit_cells;
        out.max_hits = info.max_hits, out.max_misses = info.max_misses, out.frames_used = info.frames_used;
        const std::size_t cells = static_cast<std::size_t>(info.width) * static_cast<std::size_t>(info.height);
        out.hits.resize(cells), out.misses.resize(cells), out.probability.resize(cells);
        if (cells)
            check(icpmi_map_live_counts(m_, out.hits.data(), out.misses.data(), out.probability.data(),
                                        static_cast<int64_t>(cells), nullptr));
        return out;
    }
    // forget the frames cast so far: the next live_update casts every used frame again
    void live_clear() { check(icpmi_map_live_clear(m_)); }
    // icpmi_map_set_ground: from here on finish's cell set, raycast, raycast_counts and live_update take as a frame's
    // hits its OBSTACLE rows instead of the grid's band on world z; clear_ground turns that off again.  Either way the
    // next live_update rebuilds.
    void set_ground(const GroundConfig &config)
    {
        const icpmi_ground_config k = detail::to_c(config);
        check(icpmi_map_set_ground(m_, &k));
    }
    void clear_ground() { check(icpmi_map_set_ground(m_, nullptr)); }
    // one frame's cached labels (GroundLabel's values), formed first if need be; needs a ground config
    std::vector<uint8_t> ground_labels(std::size_t frame)
    {
        int64_t n = 0;
        check(icpmi_map_ground_labels(m_, static_cast<int64_t>(frame), nullptr, 0, &n));
        std::vector<uint8_t> out(static_cast<std::size_t>(n));
        if (n) check(icpmi_map_ground_labels(m_, static_cast<int64_t>(frame), out.data(), n, &n));
        return out;
    }
    // The static map (icpmi_map_world_static): global_map() / recent_clouds()'s points without the rows whose cells the
    // counts outvote, frames [first, used), frame then row order, each bit for bit the point global_map() holds for that
    // row.  The live counts are brought up to date first, as by live_update(poses, grid).  The default grid's band holds
    // no car roof when the sensor is the origin of z: see icp_mi355x.h.
    PointCloud world_static(const std::vector<Transformation> &poses, const OccupancyGridConfig &grid, const StaticRule &rule = StaticRule(),
                            std::size_t first = 0, StaticInfo *info = nullptr)
    {
        const std::vector<double> P = flatten(poses);
        const icpmi_grid_config g = detail::to_c(grid);
        const icpmi_static_rule r{rule.min_probability, rule.min_observations, 0};
        icpmi_static_info si{};
        int64_t n = 0;
        std::size_t cap = 0; // one call, so that info->live is that call's update
        for (std::size_t i = first; i < rows_.size() && i < poses.size(); ++i) cap += rows_[i];
        std::vector<double> out(3 * std::max<std::size_t>(cap, 1));
        check(icpmi_map_world_static(m_, P.data(), static_cast<int64_t>(poses.size()), &g, &r, static_cast<int64_t>(first), out.data(),
                                     static_cast<int64_t>(cap), &n, &si));
        out.resize(3 * static_cast<std::size_t>(n));
        if (info) *info = from_c(si);
        return PointCloud(std::move(out));
    }
    // finish()'s published map over the kept rows of all used frames (icpmi_map_finish_static).  The context's cell set
    // is not touched.
    PointCloud finish_static(const std::vector<Transformation> &poses, const OccupancyGridConfig &grid, const StaticRule &rule,
                             double voxel_size, StaticInfo *info = nullptr)
    {
        const std::vector<double> P = flatten(poses);
        const icpmi_grid_config g = detail::to_c(grid);
        const icpmi_static_rule r{rule.min_probability, rule.min_observations, 0};
        std::size_t rows = 0;
        for (std::size_t i = 0; i < rows_.size() && i < poses.size(); ++i) rows += rows_[i];
        std::vector<double> out(3 * std::max<std::size_t>(rows, 1));
        icpmi_static_info si{};
        int64_t n = 0;
        check(icpmi_map_finish_static(m_, P.data(), static_cast<int64_t>(poses.size()), &g, &r, voxel_size, out.data(),
                                      static_cast<int64_t>(rows), &n, &si));
        out.resize(3 * static_cast<std::size_t>(n));
        if (info) *info = from_c(si);
        return PointCloud(std::move(out));
    }
    // one frame's labels (0 kept and does not vote, 1 kept and votes, 2 dropped) as the last world_static or
    // finish_static left them
    std::vector<uint8_t> static_labels(std::size_t frame)
    {
        int64_t n = 0;
        check(icpmi_map_static_labels(m_, static_cast<int64_t>(frame), nullptr, 0, &n));
        std::vector<uint8_t> out(static_cast<std::size_t>(n));
        if (n) check(icpmi_map_static_labels(m_, static_cast<int64_t>(frame), out.data(), n, &n));
        return out;
    }
    icpmi_map *get() const { return m_; }
    Context *context() const { return ctx_; }

private:
    void check(int rc) const
    {
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
    }
    int64_t points() const
    {
        int64_t n = 0;
        check(icpmi_map_size(m_, nullptr, &n));
        return n;
    }
    static StaticInfo from_c(const icpmi_static_info &si)
    {
        StaticInfo out;
        out.rows = si.rows, out.voting = si.voting, out.dropped = si.dropped, out.kept = si.kept;
        out.live.frames_cast = si.live.frames_cast;
        out.live.rebuilt = si.live.rebuilt != 0, out.live.moved = si.live.moved != 0;
        out.live.plane_x0 = si.live.plane_x0, out.live.plane_y0 = si.live.plane_y0;
        out.live.plane_w = si.live.plane_w, out.live.plane_h = si.live.plane_h;
        return out;
    }
    static std::vector<double> flatten(const std::vector<Transformation> &poses)
    {
        std::vector<double> P;
        P.reserve(16 * poses.size());
        for (const Transformation &T : poses) P.insert(P.end(), T.matrix().begin(), T.matrix().end());
        return P;
    }
    std::vector<double> world(const std::vector<Transformation> &poses, std::size_t first) const
    {
        const std::vector<double> P = flatten(poses);
        int64_t n = 0;
        check(icpmi_map_world(m_, P.data(), static_cast<int64_t>(poses.size()), static_cast<int64_t>(first), nullptr, 0, &n));
        std::vector<double> out(3 * static_cast<std::size_t>(n));
        if (n) check(icpmi_map_world(m_, P.data(), static_cast<int64_t>(poses.size()), static_cast<int64_t>(first), out.data(), n, &n));
        return out;
    }
    Context *ctx_;
    icpmi_map *m_ = nullptr;
    std::vector<std::size_t> rows_; // rows per frame
};

// The sliding voxel map of scan-to-local-map odometry (icpmi_local_map_*; not in the reference node, which registers
// each scan against the one before it, slam_node.cpp:132-138): the recent scans in one frame, at most one point per
// voxel, kept on the device as the registration target.  icp_mi355x.h has the table's rules.  max_range must cover
// the sensor's range.  Non-copyable, movable; destroy it before its context.
struct LocalMapConfig {
    double voxel_size = 0.5;
    double max_range = 100.0;
    std::int64_t capacity = std::int64_t(1) << 20; // rows, 64 bytes of device memory each
};
struct LocalMapInfo { // of one add
    long long rows = 0, inserted = 0, evicted = 0, dropped = 0, merged = 0;
};

class LocalMap {
public:
    explicit LocalMap(const LocalMapConfig &config = LocalMapConfig(), Context *ctx = nullptr)
        : ctx_(ctx ? ctx : &default_context()), config_(config)
    {
        icpmi_local_map_config c;
        icpmi_local_map_config_default(&c);
        c.voxel_size = config.voxel_size;
        c.max_range = config.max_range;
        c.capacity = config.capacity;
        check(icpmi_local_map_create(ctx_->get(), &c, &m_));
    }
    ~LocalMap() { icpmi_local_map_destroy(m_); }
    LocalMap(const LocalMap &) = delete;
    LocalMap &operator=(const LocalMap &) = delete;
    LocalMap(LocalMap &&o) noexcept : ctx_(o.ctx_), config_(o.config_), m_(o.m_) { o.m_ = nullptr; }
    LocalMap &operator=(LocalMap &&o) noexcept
    {
        if (this != &o) {
            icpmi_local_map_destroy(m_);
            ctx_ = o.ctx_;
            config_ = o.config_;
            m_ = o.m_;
            o.m_ = nullptr;
        }
        return *this;
    }
    const LocalMapConfig &config() const { return config_; }

    // evict what is out of range of `pose`, insert the scan's new voxels, merge
    LocalMapInfo add(const PointCloud &scan, const Transformation &pose)
    {
        icpmi_local_map_info i{};
        check(icpmi_local_map_add(m_, scan.data(), static_cast<int64_t>(scan.size()), pose.matrix().data(), &i));
        return info(i);
    }
    // the same for the scan an OdometryStream on this context pushed last, without a trip through the host
    LocalMapInfo add_stream_frame(const Transformation &pose)
    {
        icpmi_local_map_info i{};
        check(icpmi_local_map_add_stream_frame(m_, pose.matrix().data(), &i));
        return info(i);
    }
    void clear() { check(icpmi_local_map_clear(m_)); }
    std::size_t size() const
    {
        int64_t n = 0;
        check(icpmi_local_map_size(m_, &n));
        return static_cast<std::size_t>(n);
    }
    // the table's points, sorted by key; keys (may be null) receives the keys
    PointCloud points(std::vector<std::uint64_t> *keys = nullptr) const
    {
        const std::size_t n = size();
        std::vector<double> xyz(3 * n);
        if (keys) keys->resize(n);
        int64_t got = 0;
        check(icpmi_local_map_points(m_, xyz.data(), keys ? keys->data() : nullptr, static_cast<int64_t>(n), &got));
        return PointCloud(std::move(xyz));
    }
    // icp_point_to_plane(scan, the table's points): config.initial_transform is the guess in the map's frame, the
    // result's transformation the scan's pose in it
    ICPResult register_scan(const PointCloud &scan, const ICPConfig &config = ICPConfig())
    {
        icpmi_config k = detail::to_c(config);
        std::vector<double> hist(static_cast<std::size_t>(config.max_iterations > 0 ? config.max_iterations : 0) + 1);
        icpmi_result r;
        check(icpmi_local_map_register(m_, scan.data(), static_cast<int64_t>(scan.size()), &k, &r, hist.data(),
                                       static_cast<int32_t>(hist.size())));
        ICPResult out;
        detail::fill(out, r, hist.data());
        return out;
    }
    RobustICPResult register_scan(const PointCloud &scan, const RobustRule &rule, const ICPConfig &config = ICPConfig())
    {
        icpmi_config k = detail::to_c(config);
        const icpmi_robust g = detail::to_c(rule);
        icpmi_robust_info i{};
        std::vector<double> hist(static_cast<std::size_t>(config.max_iterations > 0 ? config.max_iterations : 0) + 1);
        icpmi_result r;
        check(icpmi_local_map_register_robust(m_, scan.data(), static_cast<int64_t>(scan.size()), &k, &g, &r, &i, hist.data(),
                                              static_cast<int32_t>(hist.size())));
        RobustICPResult out;
        detail::fill(out, r, hist.data());
        out.weight_sum = i.weight_sum;
        out.pairs = i.pairs;
        out.rows = i.rows;
        return out;
    }

private:
    void check(int rc) const
    {
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
    }
    static LocalMapInfo info(const icpmi_local_map_info &i)
    {
        LocalMapInfo o;
        o.rows = i.rows;
        o.inserted = i.inserted;
        o.evicted = i.evicted;
        o.dropped = i.dropped;
        o.merged = i.merged;
        return o;
    }
    Context *ctx_;
    LocalMapConfig config_;
    icpmi_local_map *m_ = nullptr;
};

// LoopClosureDetector with its database on the device, as an index over a GlobalMap's frames (icpmi_loop_*): an
// entry is a store frame with the node's frame_idx as its label, so the node calls
//     map.add_stream_frame(); loop.addFrame(map.frames() - 1, frame_idx);
// and the scan never visits the host.  Holds no clouds and no descriptors; detect() returns what LoopClosureDetector
// returns over the same clouds.  Non-copyable, movable; destroy it before its map.
class StoreLoopClosureDetector {
public:
    explicit StoreLoopClosureDetector(GlobalMap &map, LoopClosureConfig config = LoopClosureConfig())
        : ctx_(map.context()), config_(config)
    {
        icpmi_loop_config c;
        icpmi_loop_config_default(&c);
        c.frame_gap = config.frame_gap;
        c.max_candidates = config.max_candidates;
        c.sc_distance_threshold = config.sc_distance_threshold;
        c.icp_fitness_threshold = config.icp_fitness_threshold;
        check(icpmi_loop_create(map.get(), &c, &l_));
        try {
            if (config.yaw_guess) check(icpmi_loop_set_yaw_guess(l_, 1));
            if (config.max_correspondence_distance > 0.0) check(icpmi_loop_set_gate(l_, config.max_correspondence_distance));
            if (config.robust_kind != 0) check(icpmi_loop_set_robust(l_, config.robust_kind, config.robust_scale));
            if (config.gicp_epsilon != 0.0) check(icpmi_loop_set_gicp(l_, config.gicp_epsilon));
            if (config.information_sigma > 0.0)
                check(icpmi_loop_set_information(l_, config.information_sigma, config.information_floor_rotation,
                                                 config.information_floor_translation));
        } catch (...) { // (a setter refused: no destructor will run for this object)
            icpmi_loop_destroy(l_);
            throw;
        }
    }
    ~StoreLoopClosureDetector() { icpmi_loop_destroy(l_); }
    StoreLoopClosureDetector(const StoreLoopClosureDetector &) = delete;
    StoreLoopClosureDetector &operator=(const StoreLoopClosureDetector &) = delete;
    StoreLoopClosureDetector(StoreLoopClosureDetector &&o) noexcept : ctx_(o.ctx_), config_(o.config_), l_(o.l_) { o.l_ = nullptr; }
    StoreLoopClosureDetector &operator=(StoreLoopClosureDetector &&o) noexcept
    {
        if (this != &o) {
            icpmi_loop_destroy(l_);
            ctx_ = o.ctx_;
            config_ = o.config_;
            l_ = o.l_;
            o.l_ = nullptr;
        }
        return *this;
    }

    void addFrame(std::size_t store_frame, int frame_idx) // loop_closure.hpp:53-60 for the store's frame
    {
        check(icpmi_loop_add_frame(l_, static_cast<int64_t>(store_frame), frame_idx));
    }
    std::vector<LoopClosureResult> detect() // loop_closure.hpp:66-126
    {
        std::vector<icpmi_loop_result> buf(static_cast<std::size_t>(std::max(config_.max_candidates, 1)));
        int64_t n = 0;
        check(icpmi_loop_detect(l_, buf.data(), static_cast<int64_t>(std::max(config_.max_candidates, 0)), &n));
        std::vector<int32_t> shifts(static_cast<std::size_t>(std::max<int64_t>(n, 1)), -1);
        int64_t ns = 0;
        check(icpmi_loop_last_shifts(l_, shifts.data(), n, &ns)); // -1 each with the guess off
        std::vector<int64_t> kept(static_cast<std::size_t>(std::max<int64_t>(n, 1)), -1);
        check(icpmi_loop_last_pairs(l_, kept.data(), n, &ns)); // -1 each with the gate and plane-to-plane off
        std::vector<double> weight(static_cast<std::size_t>(std::max<int64_t>(n, 1)), -1.0);
        check(icpmi_loop_last_weights(l_, weight.data(), n, &ns)); // -1 each with the weights off
        std::vector<double> infos(36 * static_cast<std::size_t>(std::max<int64_t>(n, 1)));
        int64_t ni = 0;
        check(icpmi_loop_last_information(l_, infos.data(), n, &ni)); // none with the setting off
        std::vector<LoopClosureResult> out;
        for (int64_t i = 0; i < n; ++i) {
            const icpmi_loop_result &r = buf[static_cast<std::size_t>(i)];
            LoopClosureResult o;
            o.weight_sum = weight[static_cast<std::size_t>(i)];
            if (i < ni) {
                std::copy(infos.begin() + 36 * i, infos.begin() + 36 * (i + 1), o.information.begin());
                o.has_information = true;
            }
            o.sector_shift = shifts[static_cast<std::size_t>(i)];
            o.pairs = kept[static_cast<std::size_t>(i)];
            o.query_frame = r.query_frame;
            o.match_frame = r.match_frame;
            std::array<double, 16> m;
            std::copy(r.transform, r.transform + 16, m.begin());
            o.transform = Transformation(m);
            o.scan_context_distance = r.scan_context_distance;
            o.icp_fitness = r.icp_fitness;
            out.push_back(o);
        }
        return out;
    }
    std::size_t size() const
    {
        int64_t n = 0;
        check(icpmi_loop_size(l_, &n));
        return static_cast<std::size_t>(n);
    }
    void clear() { check(icpmi_loop_clear(l_)); } // the store is untouched
    std::vector<double> descriptor(std::size_t entry) const // 20 x 60, row-major
    {
        std::vector<double> d(static_cast<std::size_t>(ICPMI_SC_RINGS) * ICPMI_SC_SECTORS);
        check(icpmi_loop_descriptor(l_, static_cast<int64_t>(entry), d.data()));
        return d;
    }
    const LoopClosureConfig &config() const { return config_; }
    icpmi_loop *get() const { return l_; }

private:
    void check(int rc) const
    {
        if (rc != ICPMI_OK) throw IcpError(rc, icpmi_last_error(ctx_->get()));
    }
    Context *ctx_;
    LoopClosureConfig config_;
    icpmi_loop *l_ = nullptr;
};

} // namespace icp_mi355x
