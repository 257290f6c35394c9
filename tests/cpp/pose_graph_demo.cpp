// Exercises the pose-graph part of the C++17 host mirror (include/icp_mi355x.hpp): the reference node's use of
// slam::PoseGraph (slam_node.cpp:66,145,163,177-185) with the mirror behind the same names.  Compiled
// -fsyntax-only -Wall -Wextra -Werror by tests/test_pose_graph_header.py.
#include <cstdio>
#include <type_traits>
#include <utility>
#include <vector>

#include "icp_mi355x.hpp"

namespace slam = icp_mi355x;

int main()
{
    slam::PoseGraphConfig config;
    config.max_iterations = 50;
    slam::PoseGraph graph(config);
    static_assert(!std::is_copy_constructible<slam::PoseGraph>::value, "PoseGraph is not copyable");
    static_assert(std::is_move_constructible<slam::PoseGraph>::value, "PoseGraph is movable");
    std::vector<slam::Transformation> poses{slam::Transformation::identity()};
    graph.addPrior(0, slam::Transformation::identity());                           // slam_node.cpp:66
    const slam::Transformation step = slam::Transformation::from_rt({1, 0, 0, 0, 1, 0, 0, 0, 1}, {1.0, 0.0, 0.0});
    for (std::size_t k = 1; k <= 20; ++k) {
        poses.push_back(poses.back());
        graph.addOdometryFactor(k - 1, k, step, 0.01);                            // :145
    }
    graph.addLoopClosure(0, 20, slam::Transformation::from_rt({1, 0, 0, 0, 1, 0, 0, 0, 1}, {19.5, 0.0, 0.0}));   // :163
    if (graph.optimize()) {                                                       // :177-185
        poses = graph.getAllPoses();
        std::printf("Optimized, error=%.2f, iterations=%d, poses=%zu, loops=%zu\n", graph.getFinalError(),
                    graph.getIterations(), graph.size(), graph.loopClosureCount());
    }
    slam::PoseGraph moved(std::move(graph));
    const slam::Transformation last = moved.getPose(20);
    std::printf("x20=%.6f\n", last(0, 3));
    return 0;
}
