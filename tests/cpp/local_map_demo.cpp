// Exercises the local-map part of the C++17 host mirror (include/icp_mi355x.hpp): scan-to-local-map odometry as a node
// would run it -- constant-velocity guess, registration against the sliding voxel map, the node's gate
// (slam_node.cpp:139-140) keeping the guess, and the add that always follows.  Compiled -fsyntax-only -Wall -Wextra
// -Werror by tests/test_local_map_header.py.
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <utility>
#include <vector>

#include "icp_mi355x.hpp"

namespace slam = icp_mi355x;

int main()
{
    slam::Context ctx;
    slam::LocalMapConfig config;
    config.max_range = 120.0; // covers the sensor's 80 m
    slam::LocalMap map(config, &ctx);
    static_assert(!std::is_copy_constructible<slam::LocalMap>::value, "LocalMap is not copyable");
    static_assert(std::is_move_constructible<slam::LocalMap>::value, "LocalMap is movable");
    const slam::PointCloud scan(std::vector<double>{1.0, 2.0, 0.5, 3.0, -1.0, 1.0, 3.1, -1.1, 1.2});
    slam::Transformation pose = slam::Transformation::identity(), delta = slam::Transformation::identity();
    slam::LocalMapInfo info = map.add(scan, pose);                                // frame 0
    for (int k = 1; k <= 3; ++k) {
        slam::ICPConfig icp;
        icp.initial_transform = pose * delta;                                     // the guess, in the map's frame
        const slam::ICPResult r = map.register_scan(scan, icp);
        const bool bad = !r.converged || r.final_error > 1.0;                     // slam_node.cpp:139-140
        const slam::Transformation next = bad ? icp.initial_transform : r.transformation;
        delta = pose.inverse() * next;
        pose = next;
        info = map.add(scan, pose);                                               // always
    }
    slam::RobustRule rule;
    const slam::RobustICPResult rr = map.register_scan(scan, rule);
    slam::OdometryStream stream(&ctx);
    stream.push(scan, 0.5, 1);
    info = map.add_stream_frame(pose);                                            // the scan kept on the device
    std::vector<std::uint64_t> keys;
    const slam::PointCloud table = map.points(&keys);
    slam::LocalMap moved(std::move(map));
    std::printf("rows=%zu keys=%zu inserted=%lld evicted=%lld dropped=%lld merged=%lld weight_sum=%g voxel=%g\n", moved.size(),
                keys.size(), info.inserted, info.evicted, info.dropped, info.merged, rr.weight_sum, moved.config().voxel_size);
    moved.clear();
    return table.size() == keys.size() ? 0 : 1;
}
