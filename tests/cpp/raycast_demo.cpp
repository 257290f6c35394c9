// Exercises the ray-cast part of the C++17 host mirror (include/icp_mi355x.hpp): the node's
// publish_occupancy_grid -> cells_to_occupancy_grid_msg (slam_node.cpp:279-297) with GlobalMap::raycast behind it, so
// that unseen space is published as unknown and not as free.  Compiled -fsyntax-only -Wall -Wextra -Werror by
// tests/test_raycast_header.py.
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
    std::vector<slam::Transformation> poses{slam::Transformation::identity()};
    const slam::PointCloud scan(std::vector<double>{4.0, 2.0, 0.5, -3.0, -1.0, 1.0});
    map.add_frame(scan);
    const slam::Transformation step = slam::Transformation::from_rt({1, 0, 0, 0, 1, 0, 0, 0, 1}, {1.0, 0.0, 0.0});
    for (int k = 1; k <= 3; ++k) {
        map.add_frame(scan);
        poses.push_back(poses.back() * step);
    }
    const slam::OccupancyRaster raster = map.raycast(poses, slam::OccupancyGridConfig());
    static_assert(std::is_same<decltype(raster.data), std::vector<int8_t>>::value, "the raster is int8, as nav_msgs/OccupancyGrid");
    static_assert(ICPMI_RAYCAST_LDS_MAX_R < ICPMI_RAYCAST_MAX_R, "both limits are in the C header");
    // the message's fields: info.resolution, info.width, info.height, info.origin.position = min * resolution, data
    std::size_t occupied = 0, free_cells = 0;
    for (const int8_t v : raster.data) occupied += v == 100, free_cells += v == 0;
    std::printf("origin=(%g, %g) %d x %d at %g m: %zu occupied, %zu free\n", raster.min_x * raster.resolution,
                raster.min_y * raster.resolution, raster.width, raster.height, raster.resolution, occupied, free_cells);
    return 0;
}
