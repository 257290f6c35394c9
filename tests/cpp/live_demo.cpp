// Exercises the live count part of the C++17 host mirror (include/icp_mi355x.hpp): the node's process_frame
// (slam_node.cpp:118-175) with GlobalMap::live_update where update_occupancy_grid stands (:152), and again after
// run_pose_graph_optimization has replaced the poses (:177-185), so that publish_occupancy_grid has the probability
// grid of every frame so far without casting them all again.  Compiled -fsyntax-only -Wall -Wextra -Werror by
// tests/test_live_header.py.
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "icp_mi355x.hpp"

namespace slam = icp_mi355x;

int main()
{
    slam::Context ctx;
    slam::GlobalMap map(&ctx);
    const slam::OccupancyGridConfig grid;
    std::vector<slam::Transformation> poses{slam::Transformation::identity()};
    const slam::PointCloud scan(std::vector<double>{4.0, 2.0, 0.5, -3.0, -1.0, 1.0});
    const slam::Transformation step = slam::Transformation::from_rt({1, 0, 0, 0, 1, 0, 0, 0, 1}, {15.0, 0.0, 0.0});
    map.add_frame(scan);
    slam::LiveUpdate u = map.live_update(poses, grid);
    int64_t cast = u.frames_cast;
    int moves = 0;
    for (int k = 1; k <= 8; ++k) {                       // process_frame: keep the scan, then its pose, then the grid
        map.add_frame(scan);
        poses.push_back(poses.back() * step);
        u = map.live_update(poses, grid);
        cast += u.frames_cast;
        moves += u.moved;
    }
    poses.back() = poses.back() * step;                  // run_pose_graph_optimization moved a pose: everything again
    u = map.live_update(poses, grid);
    static_assert(std::is_same<decltype(u.frames_cast), int64_t>::value && std::is_same<decltype(u.rebuilt), bool>::value,
                  "the update says what it cost");
    static_assert(sizeof(icpmi_live_info) == sizeof(icpmi_counts_info) + 32, "the C struct has no hidden padding");
    const slam::OccupancyCounts counts = map.live_counts();
    static_assert(std::is_same<decltype(counts.probability), std::vector<int8_t>>::value, "int8, as nav_msgs/OccupancyGrid");
    std::printf("%lld frames cast one by one, %d plane moves, then %lld again (rebuilt=%d); plane %d x %d at (%d, %d); %lld observed\n",
                static_cast<long long>(cast), moves, static_cast<long long>(u.frames_cast), static_cast<int>(u.rebuilt), u.plane_w,
                u.plane_h, u.plane_x0, u.plane_y0, static_cast<long long>(counts.n_observed));
    map.live_clear();
    return map.live_counts().hits.empty() ? 0 : 1;
}
