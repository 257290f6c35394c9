// Exercises the hit / miss count part of the C++17 host mirror (include/icp_mi355x.hpp): the node's
// publish_occupancy_grid -> cells_to_occupancy_grid_msg (slam_node.cpp:279-297) with GlobalMap::raycast_counts behind
// it, so that the message's data says how often a cell was seen occupied (0..100, -1 unknown) and one stray return
// does not block a cell for good.  Compiled -fsyntax-only -Wall -Wextra -Werror by tests/test_counts_header.py.
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "icp_mi355x.hpp"

namespace slam = icp_mi355x;

// nav_msgs/OccupancyGrid, as far as the node fills it
struct OccupancyGridMsg {
    double resolution = 0.0, origin_x = 0.0, origin_y = 0.0;
    uint32_t width = 0, height = 0;
    std::vector<int8_t> data;
};

static OccupancyGridMsg cells_to_occupancy_grid_msg(const slam::OccupancyCounts &counts)
{
    OccupancyGridMsg msg;
    msg.resolution = counts.resolution;
    msg.width = static_cast<uint32_t>(counts.width);
    msg.height = static_cast<uint32_t>(counts.height);
    msg.origin_x = counts.min_x * counts.resolution;
    msg.origin_y = counts.min_y * counts.resolution;
    msg.data = counts.probability;
    return msg;
}

int main()
{
    slam::Context ctx;
    slam::GlobalMap map(&ctx);
    std::vector<slam::Transformation> poses{slam::Transformation::identity()};
    const slam::PointCloud scan(std::vector<double>{4.0, 2.0, 0.5, -3.0, -1.0, 1.0});
    map.add_frame(scan);
    const slam::Transformation step = slam::Transformation::from_rt({1, 0, 0, 0, 1, 0, 0, 0, 1}, {1.0, 0.0, 0.0});
    for (int k = 1; k <= 3; ++k) {
        map.add_frame(scan);
        poses.push_back(poses.back() * step);
    }
    const slam::OccupancyCounts counts = map.raycast_counts(poses, slam::OccupancyGridConfig());
    static_assert(std::is_same<decltype(counts.hits), std::vector<uint16_t>>::value &&
                      std::is_same<decltype(counts.misses), std::vector<uint16_t>>::value,
                  "a count is 16 bits: ICPMI_RAYCOUNT_MAX_FRAMES frames add at most 1 each");
    static_assert(std::is_same<decltype(counts.probability), std::vector<int8_t>>::value, "int8, as nav_msgs/OccupancyGrid");
    static_assert(ICPMI_RAYCOUNT_MAX_FRAMES == UINT16_MAX && ICPMI_RAYCOUNT_LDS_MAX_R < ICPMI_RAYCAST_LDS_MAX_R,
                  "both limits are in the C header");
    static_assert(sizeof(icpmi_counts_info) == 56, "the C struct has no hidden padding");
    const OccupancyGridMsg msg = cells_to_occupancy_grid_msg(counts);
    std::size_t certain = 0, doubtful = 0;
    for (const int8_t v : msg.data) certain += v == 100 || v == 0, doubtful += v > 0 && v < 100;
    std::printf("origin=(%g, %g) %u x %u at %g m: %lld observed cells of %d frames, %zu certain, %zu in between; hits <= %d, misses <= %d\n",
                msg.origin_x, msg.origin_y, msg.width, msg.height, msg.resolution, static_cast<long long>(counts.n_observed),
                counts.frames_used, certain, doubtful, counts.max_hits, counts.max_misses);
    return 0;
}
