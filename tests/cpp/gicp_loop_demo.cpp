// Exercises plane-to-plane loop verification of the C++17 host mirror (include/icp_mi355x.hpp: GicpRule::small_form,
// align_gicp_batch, LoopClosureConfig::gicp_epsilon) on the GPU:
//   gicp_loop_demo <out.f64> <frame_gap> <sc_distance_threshold> <icp_fitness_threshold> <max_candidates> <yaw_guess 0|1>
//                  <max_correspondence_distance> <gicp_epsilon> <label0> <cloud0.f64> <label1> <cloud1.f64> ...
// adds the clouds (row-major N x 3 fp64 files) with their labels to a LoopClosureDetector and, as frames of a GlobalMap,
// to a StoreLoopClosureDetector, calls detect() on both after every frame like SlamNode does, prints every closure, and
// writes, as fp64, first the host detector's closures, then the store detector's:
//   [results, per result: query_frame, match_frame, sector_shift, pairs, scan_context_distance, icp_fitness, transform(16)]
// then one align_gicp(last cloud -> first cloud) in the small form under the same rule from the identity with 30
// iterations, and the same problem twice through align_gicp_batch:
//   3 x [pairs, rows, converged, num_iterations, final_error, transform(16)]
// tests/test_gpu_gicp_small.py compares every number with the Python mirror.
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

static_assert(sizeof(icpmi_gicp) == 24 && offsetof(icpmi_gicp, epsilon) == 0 && offsetof(icpmi_gicp, max_distance) == 8 &&
                  offsetof(icpmi_gicp, reserved) == 16,
              "icpmi_gicp keeps its layout");
static_assert(ICPMI_GICP_FORM_SMALL == 1, "the form's bit");

static void append(std::vector<double> &out, const char *who, const std::vector<im::LoopClosureResult> &found)
{
    out.push_back(static_cast<double>(found.size()));
    for (const im::LoopClosureResult &r : found) {
        std::printf("%s: query %d match %d shift %d pairs %lld distance %.6f fitness %.6f\n", who, r.query_frame, r.match_frame,
                    r.sector_shift, r.pairs, r.scan_context_distance, r.icp_fitness);
        out.push_back(r.query_frame);
        out.push_back(r.match_frame);
        out.push_back(r.sector_shift);
        out.push_back(static_cast<double>(r.pairs));
        out.push_back(r.scan_context_distance);
        out.push_back(r.icp_fitness);
        out.insert(out.end(), r.transform.matrix().begin(), r.transform.matrix().end());
    }
}

static void append(std::vector<double> &out, const im::GicpICPResult &g)
{
    std::printf("align_gicp: pairs %lld of %lld, %d iterations, final error %.6f\n", g.pairs, g.rows, g.num_iterations, g.final_error);
    out.push_back(static_cast<double>(g.pairs));
    out.push_back(static_cast<double>(g.rows));
    out.push_back(g.converged ? 1.0 : 0.0);
    out.push_back(g.num_iterations);
    out.push_back(g.final_error);
    out.insert(out.end(), g.transformation.matrix().begin(), g.transformation.matrix().end());
}

int main(int argc, char **argv)
{
    if (argc < 11 || (argc - 9) % 2 != 0) {
        std::fprintf(stderr, "usage: %s out.f64 frame_gap sc_threshold icp_threshold max_candidates yaw_guess max_distance gicp_epsilon (label cloud.f64)...\n",
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
        cfg.gicp_epsilon = std::atof(argv[8]);
        im::Context &ctx = im::default_context();
        im::LoopClosureDetector host(cfg, &ctx);
        im::GlobalMap map(&ctx);
        im::StoreLoopClosureDetector store(map, cfg);
        std::vector<im::LoopClosureResult> found_host, found_store;
        std::vector<im::PointCloud> clouds;
        for (int k = 9; k + 1 < argc; k += 2) {
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
        im::ICPConfig icp;
        icp.max_iterations = 30;
        im::GicpRule rule;
        rule.epsilon = cfg.gicp_epsilon;
        rule.max_distance = cfg.max_correspondence_distance;
        rule.small_form = true;
        append(out, im::align_gicp(clouds.back(), clouds.front(), rule, icp));
        for (const im::GicpICPResult &g : im::align_gicp_batch(ctx, clouds.back(), {&clouds.front(), &clouds.front()}, rule, icp))
            append(out, g);
        std::ofstream f(argv[1], std::ios::binary);
        f.write(reinterpret_cast<const char *>(out.data()), static_cast<std::streamsize>(out.size() * sizeof(double)));
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "gicp_loop_demo: %s\n", e.what());
        return 1;
    }
}
