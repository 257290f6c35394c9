// Exercises the store loop-closure part of the C++17 host mirror (include/icp_mi355x.hpp): the reference node's
// process_frame with the scan kept on the device from the stream, through the global map, to the detector and the
// pose graph (slam_node.cpp:118-175), and nothing downloaded for the detector.  Compiled -fsyntax-only -Wall -Wextra
// -Werror by tests/test_loop_store_header.py.
#include <cstdio>
#include <type_traits>
#include <utility>
#include <vector>

#include "icp_mi355x.hpp"

namespace slam = icp_mi355x;

int main()
{
    slam::Context ctx;
    slam::GlobalMap map(&ctx);
    slam::LoopClosureConfig loop_cfg;                                              // slam_node.cpp:77-80
    loop_cfg.frame_gap = 50;
    loop_cfg.sc_distance_threshold = 0.2;
    loop_cfg.icp_fitness_threshold = 0.3;
    slam::StoreLoopClosureDetector loop(map, loop_cfg);
    static_assert(!std::is_copy_constructible<slam::StoreLoopClosureDetector>::value, "not copyable");
    static_assert(std::is_move_constructible<slam::StoreLoopClosureDetector>::value, "movable");
    slam::PoseGraph graph(slam::PoseGraphConfig(), &ctx);
    slam::OdometryStream stream(&ctx);
    std::vector<slam::Transformation> poses{slam::Transformation::identity()};
    graph.addPrior(0, poses.front());                                              // :66
    const slam::PointCloud scan(std::vector<double>{1.0, 2.0, 0.5, 3.0, -1.0, 1.0});
    stream.push(scan, 0.5, 1);
    map.add_stream_frame();                                                       // :71
    for (int k = 1; k <= 120; ++k) {
        const slam::OdometryStream::Step st = stream.push(scan, 0.5, 1);          // :122-140
        map.add_stream_frame();                                                   // :123, the scan kept on the device
        if (!st.registered) {                                                     // :125-130
            poses.push_back(poses.back());
            continue;
        }
        poses.push_back(poses.back() * st.result.transformation);
        graph.addOdometryFactor(poses.size() - 2, poses.size() - 1, st.result.transformation, st.result.final_error);
        loop.addFrame(map.frames() - 1, k);                                       // :159, no current_scan() download
        bool pending = false;
        if (k % 10 == 0 && k > 50)                                                // :160
            for (const slam::LoopClosureResult &c : loop.detect()) {              // :161-166
                graph.addLoopClosure(static_cast<std::size_t>(c.match_frame), static_cast<std::size_t>(c.query_frame),
                                     c.transform);
                pending = true;
            }
        if (pending && graph.optimize()) poses = graph.getAllPoses();             // :112-115, :177-185
    }
    const std::vector<double> d = loop.descriptor(0);
    slam::StoreLoopClosureDetector moved(std::move(loop));
    std::printf("entries=%zu frames=%zu descriptor=%zu loops=%zu\n", moved.size(), map.frames(), d.size(),
                graph.loopClosureCount());
    moved.clear();
    return 0;
}
