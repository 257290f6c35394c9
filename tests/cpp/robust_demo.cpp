// Exercises the robust row weights of the C++17 host mirror (include/icp_mi355x.hpp: align_robust, RobustRule,
// LoopClosureConfig::robust_kind / robust_scale, LoopClosureResult::weight_sum) on the GPU:
//   robust_demo <out.f64> <frame_gap> <sc_distance_threshold> <icp_fitness_threshold> <max_candidates> <yaw_guess 0|1>
//               <max_correspondence_distance> <robust_kind> <robust_scale> <label0> <cloud0.f64> <label1> <cloud1.f64> ...
// adds the clouds (row-major N x 3 fp64 files) with their labels to a LoopClosureDetector and, as frames of a GlobalMap,
// to a StoreLoopClosureDetector, calls detect() on both after every frame like SlamNode does, prints every closure, and
// writes, as fp64, first the host detector's closures, then the store detector's:
//   [results, per result: query_frame, match_frame, sector_shift, pairs, weight_sum, scan_context_distance, icp_fitness,
//    transform(16)]
// and last one align_robust(last cloud -> first cloud) under the same rule from the identity with 30 iterations:
//   [weight_sum, pairs, rows, converged, num_iterations, final_error, transform(16)]
// tests/test_gpu_robust.py compares every number with the Python mirror.  The static assertions pin the layout of the
// structs that existed before the weights to what it was, and of the two new ones (tests/test_robust_header.py compiles
// this file with -fsyntax-only).
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "icp_mi355x.hpp"

static std::vector<double> read_f64(const char *path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    const std::streamsize bytes = f.tellg();
    f.seekg(0);
    std::vector<double> v(static_cast<std::size_t>(bytes) / sizeof(double));
    f.read(reinterpret_cast<char *>(v.data()), bytes);
    return v;
}

namespace im = icp_mi355x;

static_assert(sizeof(icpmi_config) == 152 && offsetof(icpmi_config, max_iterations) == 0 && offsetof(icpmi_config, reserved) == 4 &&
                  offsetof(icpmi_config, tolerance) == 8 && offsetof(icpmi_config, min_error) == 16 &&
                  offsetof(icpmi_config, initial_transform) == 24,
              "icpmi_config keeps its layout");
static_assert(sizeof(icpmi_result) == 152 && offsetof(icpmi_result, transformation) == 0 && offsetof(icpmi_result, converged) == 128 &&
                  offsetof(icpmi_result, num_iterations) == 132 && offsetof(icpmi_result, final_error) == 136 &&
                  offsetof(icpmi_result, history_len) == 144 && offsetof(icpmi_result, loop_iterations) == 148,
              "icpmi_result keeps its layout");
static_assert(sizeof(icpmi_gate) == 16 && offsetof(icpmi_gate, max_distance) == 0 && offsetof(icpmi_gate, reserved) == 8 &&
                  sizeof(icpmi_gate_info) == 16 && offsetof(icpmi_gate_info, pairs) == 0 && offsetof(icpmi_gate_info, rows) == 8,
              "the gate's structs keep their layout");
static_assert(sizeof(icpmi_stream_info) == 24 && offsetof(icpmi_stream_info, status) == 0 && offsetof(icpmi_stream_info, reserved) == 4 &&
                  offsetof(icpmi_stream_info, n_filtered) == 8 && offsetof(icpmi_stream_info, n_target) == 16,
              "icpmi_stream_info keeps its layout");
static_assert(sizeof(icpmi_robust) == 24 && offsetof(icpmi_robust, kind) == 0 && offsetof(icpmi_robust, reserved) == 4 &&
                  offsetof(icpmi_robust, scale) == 8 && offsetof(icpmi_robust, max_distance) == 16,
              "icpmi_robust");
static_assert(sizeof(icpmi_robust_info) == 24 && offsetof(icpmi_robust_info, weight_sum) == 0 && offsetof(icpmi_robust_info, pairs) == 8 &&
                  offsetof(icpmi_robust_info, rows) == 16,
              "icpmi_robust_info");
static_assert(ICPMI_ROBUST_HUBER == 1 && ICPMI_ROBUST_GEMAN_MCCLURE == 2, "the kinds");

static void append(std::vector<double> &out, const char *who, const std::vector<im::LoopClosureResult> &found)
{
    out.push_back(static_cast<double>(found.size()));
    for (const im::LoopClosureResult &r : found) {
        std::printf("%s: query %d match %d shift %d pairs %lld weight sum %.6f distance %.6f fitness %.6f\n", who, r.query_frame,
                    r.match_frame, r.sector_shift, r.pairs, r.weight_sum, r.scan_context_distance, r.icp_fitness);
        out.push_back(r.query_frame);
        out.push_back(r.match_frame);
        out.push_back(r.sector_shift);
        out.push_back(static_cast<double>(r.pairs));
        out.push_back(r.weight_sum);
        out.push_back(r.scan_context_distance);
        out.push_back(r.icp_fitness);
        out.insert(out.end(), r.transform.matrix().begin(), r.transform.matrix().end());
    }
}

int main(int argc, char **argv)
{
    if (argc < 12 || (argc - 10) % 2 != 0) {
        std::fprintf(stderr, "usage: %s out.f64 frame_gap sc_threshold icp_threshold max_candidates yaw_guess max_distance robust_kind robust_scale (label cloud.f64)...\n",
                     argv[0]);
        return 2;
    }
    try {
        im::LoopClosureConfig cfg;                                   // loop_closure.hpp:14-19
        cfg.frame_gap = std::atoi(argv[2]);
        cfg.sc_distance_threshold = std::atof(argv[3]);
        cfg.icp_fitness_threshold = std::atof(argv[4]);
        cfg.max_candidates = std::atoi(argv[5]);
        cfg.yaw_guess = std::atoi(argv[6]) != 0;
        cfg.max_correspondence_distance = std::atof(argv[7]);
        cfg.robust_kind = std::atoi(argv[8]);
        cfg.robust_scale = std::atof(argv[9]);
        im::Context &ctx = im::default_context();
        im::LoopClosureDetector host(cfg, &ctx);
        im::GlobalMap map(&ctx);
        im::StoreLoopClosureDetector store(map, cfg);
        std::vector<im::LoopClosureResult> found_host, found_store;
        std::vector<im::PointCloud> clouds;
        for (int k = 10; k + 1 < argc; k += 2) {
            const int label = std::atoi(argv[k]);
            const im::PointCloud cloud(read_f64(argv[k + 1]));
            host.addFrame(cloud, label);                             // slam_node.cpp:159
            map.add_frame(cloud);
            store.addFrame(map.frames() - 1, label);
            clouds.push_back(cloud.copy());
            for (const im::LoopClosureResult &r : host.detect()) found_host.push_back(r);     // :161
            for (const im::LoopClosureResult &r : store.detect()) found_store.push_back(r);
        }
        std::vector<double> out;
        append(out, "host ", found_host);
        append(out, "store", found_store);
        if (cfg.robust_kind != 0) {
            im::ICPConfig icp;
            icp.max_iterations = 30;
            im::RobustRule rule;
            rule.kind = cfg.robust_kind;
            rule.scale = cfg.robust_scale;
            rule.max_distance = cfg.max_correspondence_distance;
            const im::RobustICPResult g = im::align_robust(clouds.back(), clouds.front(), rule, icp);
            std::printf("align_robust: weight sum %.6f, pairs %lld of %lld, %d iterations, final error %.6f\n", g.weight_sum, g.pairs,
                        g.rows, g.num_iterations, g.final_error);
            out.push_back(g.weight_sum);
            out.push_back(static_cast<double>(g.pairs));
            out.push_back(static_cast<double>(g.rows));
            out.push_back(g.converged ? 1.0 : 0.0);
            out.push_back(g.num_iterations);
            out.push_back(g.final_error);
            out.insert(out.end(), g.transformation.matrix().begin(), g.transformation.matrix().end());
            // the stream's mirror compiles and takes the rule (no frame is pushed here)
            im::OdometryStream stream(&ctx);
            stream.set_robust(rule);
            stream.clear_robust();
        }
        std::ofstream f(argv[1], std::ios::binary);
        f.write(reinterpret_cast<const char *>(out.data()), static_cast<std::streamsize>(out.size() * sizeof(double)));
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "robust_demo: %s\n", e.what());
        return 1;
    }
}
