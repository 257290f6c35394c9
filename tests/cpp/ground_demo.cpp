// Exercises the ground-segmentation part of the C++17 host mirror (include/icp_mi355x.hpp): a scan labelled on its
// own (ground_segment), and the node's occupancy message built from the kept scans' OBSTACLE rows
// (GlobalMap::set_ground) instead of the band on world z, so that a climbing road is not published as a wall.
// Compiled -fsyntax-only -Wall -Wextra -Werror by tests/test_ground_header.py.
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "icp_mi355x.hpp"

namespace slam = icp_mi355x;

int main()
{
    slam::Context ctx;
    // a strip of road ahead of the sensor and a post on it
    std::vector<double> rows;
    for (int k = 1; k <= 20; ++k) rows.insert(rows.end(), {1.0 * k, 0.25, -1.73});
    for (int k = 0; k < 8; ++k) rows.insert(rows.end(), {5.25, 0.3, -1.4 + 0.25 * k});
    const slam::PointCloud scan(rows);

    slam::GroundConfig config;
    config.max_slope = 0.1;
    const slam::GroundSegmentation seg = slam::ground_segment(ctx, scan, config);
    static_assert(std::is_same<decltype(seg.labels), std::vector<uint8_t>>::value, "one byte per row");
    static_assert(ICPMI_GROUND_OBSTACLE == 0 && ICPMI_GROUND_GROUND == 1 && ICPMI_GROUND_IGNORED == 2, "the C header's labels");
    static_assert(static_cast<int>(slam::GroundLabel::Obstacle) == ICPMI_GROUND_OBSTACLE, "the mirror's are the same");
    static_assert(80 * 180 <= ICPMI_GROUND_MAX_BINS, "the default grid fits");
    static_assert(sizeof(icpmi_ground_config) == 72 && sizeof(icpmi_ground_info) == 32, "the C structs have no hidden padding");
    std::size_t obstacles = 0;
    for (const uint8_t l : seg.labels) obstacles += l == static_cast<uint8_t>(slam::GroundLabel::Obstacle);
    std::printf("%zu rows: %lld ground, %lld obstacle, %lld ignored; %lld bins followed; %zu bins\n", seg.labels.size(),
                static_cast<long long>(seg.n_ground), static_cast<long long>(seg.n_obstacle), static_cast<long long>(seg.n_ignored),
                static_cast<long long>(seg.bins_accepted), seg.ground_z.size());

    slam::GlobalMap map(&ctx);
    map.set_ground(config);
    std::vector<slam::Transformation> poses{slam::Transformation::identity()};
    map.add_frame(scan);
    const std::vector<uint8_t> cached = map.ground_labels(0);
    const slam::OccupancyCounts counts = map.raycast_counts(poses, slam::OccupancyGridConfig());
    const slam::LiveUpdate live = map.live_update(poses, slam::OccupancyGridConfig());
    map.clear_ground();
    const slam::OccupancyCounts banded = map.raycast_counts(poses, slam::OccupancyGridConfig());
    std::printf("%s; %lld hit cells from the labels, %lld from the band; %lld frame(s) cast live\n",
                cached == seg.labels && obstacles == static_cast<std::size_t>(seg.n_obstacle) ? "labels agree" : "labels differ",
                static_cast<long long>(counts.n_hit_cells), static_cast<long long>(banded.n_hit_cells),
                static_cast<long long>(live.frames_cast));
    return 0;
}
