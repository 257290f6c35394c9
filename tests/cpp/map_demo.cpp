// Exercises the global-map part of the C++17 host mirror (include/icp_mi355x.hpp): the reference node's
// run_pose_graph_optimization -> rebuild_recent_clouds and build_final_global_map -> rebuild_occupancy_grid ->
// publish_global_map (slam_node.cpp:71,123,177-209,223-238) with the mirror behind them.  Compiled
// -fsyntax-only -Wall -Wextra -Werror by tests/test_map_header.py.
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
    static_assert(!std::is_copy_constructible<slam::GlobalMap>::value, "GlobalMap is not copyable");
    static_assert(std::is_move_constructible<slam::GlobalMap>::value, "GlobalMap is movable");
    slam::PoseGraph graph(slam::PoseGraphConfig(), &ctx);
    slam::OdometryStream stream(&ctx);
    std::vector<slam::Transformation> poses{slam::Transformation::identity()};
    graph.addPrior(0, poses.front());                                              // slam_node.cpp:66
    const slam::PointCloud scan(std::vector<double>{1.0, 2.0, 0.5, 3.0, -1.0, 1.0});
    map.add_frame(scan);                                                          // :71
    const slam::Transformation step = slam::Transformation::from_rt({1, 0, 0, 0, 1, 0, 0, 0, 1}, {1.0, 0.0, 0.0});
    for (std::size_t k = 1; k <= 30; ++k) {
        stream.push(scan, 0.5, 1);
        map.add_stream_frame();                                                   // :123, the scan kept on the device
        poses.push_back(poses.back() * step);
        graph.addOdometryFactor(k - 1, k, step, 0.01);                            // :145
    }
    std::vector<slam::PointCloud> recent_clouds_world;
    if (graph.optimize()) {                                                       // run_pose_graph_optimization, :177-185
        poses = graph.getAllPoses();
        recent_clouds_world = map.recent_clouds(poses);                           // rebuild_recent_clouds, :187-194
    }
    const slam::PointCloud global_map_points = map.global_map(poses);            // build_final_global_map, :196-209
    slam::OccupancyGrid grid(slam::OccupancyGridConfig(), &ctx);
    const slam::PointCloud published = map.finish(poses, grid.config(), 2 * 0.5); // :223-229, :235-238
    const std::vector<slam::GridCell> cells = grid.cells();                       // the rebuilt occupied_cells_
    slam::GlobalMap moved(std::move(map));
    std::printf("frames=%zu recent=%zu global=%zu published=%zu cells=%zu\n", moved.frames(), recent_clouds_world.size(),
                global_map_points.size(), published.size(), cells.size());
    return 0;
}
