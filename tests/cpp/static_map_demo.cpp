// Exercises the static-map part of the C++17 host mirror (include/icp_mi355x.hpp): a node that publishes, every few
// frames, its recent clouds without what moved (GlobalMap::world_static where rebuild_recent_clouds stands,
// slam_node.cpp:187-194) and at the end the published map without it (GlobalMap::finish_static where publish_global_map
// stands, :235-238).  Each call brings the live counts up to date first, so only the new frames are cast.  Compiled
// -fsyntax-only -Wall -Wextra -Werror by tests/test_static_map_header.py.
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
    slam::OccupancyGridConfig grid;
    grid.height_min = -1.4, grid.height_max = 0.5;      // a band that holds a car's roof with the sensor at z = 0
    slam::StaticRule rule;
    static_assert(std::is_same<decltype(rule.min_probability), int32_t>::value, "the C struct's types");
    static_assert(sizeof(icpmi_static_rule) == 16 && sizeof(icpmi_static_info) == 32 + sizeof(icpmi_live_info), "no hidden padding");
    if (rule.min_probability != ICPMI_STATIC_MIN_PROBABILITY_DEFAULT || rule.min_observations != ICPMI_STATIC_MIN_OBSERVATIONS_DEFAULT) return 1;
    std::vector<slam::Transformation> poses{slam::Transformation::identity()};
    const slam::PointCloud scan(std::vector<double>{4.0, 2.0, 0.1, -3.0, -1.0, -0.5});
    const slam::Transformation step = slam::Transformation::from_rt({1, 0, 0, 0, 1, 0, 0, 0, 1}, {2.0, 0.0, 0.0});
    map.add_frame(scan);
    slam::StaticInfo info;
    int64_t cast = 0;
    std::size_t published_rows = 0;
    for (int k = 1; k <= 8; ++k) {
        map.add_frame(scan);
        poses.push_back(poses.back() * step);
        if (k % 4) continue;
        const std::size_t first = map.frames() > slam::GlobalMap::kMaxRecentClouds ? map.frames() - slam::GlobalMap::kMaxRecentClouds : 0;
        const slam::PointCloud recent = map.world_static(poses, grid, rule, first, &info);
        cast += info.live.frames_cast;                   // four new frames each time: nothing is cast twice
        published_rows = recent.size();
    }
    const std::vector<uint8_t> labels = map.static_labels(0);
    const slam::PointCloud published = map.finish_static(poses, grid, rule, 1.0, &info);
    static_assert(std::is_same<decltype(info.dropped), int64_t>::value && std::is_same<decltype(info.live.rebuilt), bool>::value,
                  "the info says what was dropped and what the counts cost");
    std::printf("%lld frames cast in all; %lld of %lld rows vote, %lld dropped, %lld kept; %zu recent rows, %zu published, %zu labels\n",
                static_cast<long long>(cast), static_cast<long long>(info.voting), static_cast<long long>(info.rows),
                static_cast<long long>(info.dropped), static_cast<long long>(info.kept), published_rows, published.size(), labels.size());
    return info.kept + info.dropped == info.rows ? 0 : 1;
}
