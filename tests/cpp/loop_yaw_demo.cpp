// Exercises the yaw guess of the C++17 host mirror (include/icp_mi355x.hpp, LoopClosureConfig::yaw_guess) on the GPU:
//   loop_yaw_demo <out.f64> <frame_gap> <sc_distance_threshold> <icp_fitness_threshold> <max_candidates> <yaw_guess 0|1>
//                 <label0> <cloud0.f64> <label1> <cloud1.f64> ...
// adds the clouds (row-major N x 3 fp64 files) with their labels to a LoopClosureDetector and, as frames of a GlobalMap,
// to a StoreLoopClosureDetector, calls detect() on both after every frame like SlamNode does, prints every closure with
// the column shift its verification started from, and writes, as fp64, first the host detector's closures, then the
// store detector's:
//   [results, per result: query_frame, match_frame, sector_shift, scan_context_distance, icp_fitness, transform(16)]
// tests/test_gpu_loop_yaw.py::test_cpp_loop_yaw_mirror compares every number with the Python mirror.
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

static void append(std::vector<double> &out, const char *who, const std::vector<im::LoopClosureResult> &found)
{
    out.push_back(static_cast<double>(found.size()));
    for (const im::LoopClosureResult &r : found) {
        std::printf("%s: query %d match %d shift %d (%.0f deg) distance %.6f fitness %.6f\n", who, r.query_frame,
                    r.match_frame, r.sector_shift, r.sector_shift < 0 ? 0.0 : 6.0 * r.sector_shift,
                    r.scan_context_distance, r.icp_fitness);
        out.push_back(r.query_frame);
        out.push_back(r.match_frame);
        out.push_back(r.sector_shift);
        out.push_back(r.scan_context_distance);
        out.push_back(r.icp_fitness);
        out.insert(out.end(), r.transform.matrix().begin(), r.transform.matrix().end());
    }
}

int main(int argc, char **argv)
{
    if (argc < 9 || (argc - 7) % 2 != 0) {
        std::fprintf(stderr, "usage: %s out.f64 frame_gap sc_threshold icp_threshold max_candidates yaw_guess (label cloud.f64)...\n",
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
        im::Context &ctx = im::default_context();
        im::LoopClosureDetector host(cfg, &ctx);
        im::GlobalMap map(&ctx);
        im::StoreLoopClosureDetector store(map, cfg);
        std::vector<im::LoopClosureResult> found_host, found_store;
        for (int k = 7; k + 1 < argc; k += 2) {
            const int label = std::atoi(argv[k]);
            const im::PointCloud cloud(read_f64(argv[k + 1]));
            host.addFrame(cloud, label);                             // slam_node.cpp:159
            map.add_frame(cloud);
            store.addFrame(map.frames() - 1, label);
            for (const im::LoopClosureResult &r : host.detect()) found_host.push_back(r);     // :161
            for (const im::LoopClosureResult &r : store.detect()) found_store.push_back(r);
        }
        std::vector<double> out;
        append(out, "host ", found_host);
        append(out, "store", found_store);
        std::ofstream f(argv[1], std::ios::binary);
        f.write(reinterpret_cast<const char *>(out.data()), static_cast<std::streamsize>(out.size() * sizeof(double)));
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "loop_yaw_demo: %s\n", e.what());
        return 1;
    }
}
