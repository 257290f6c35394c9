// Exercises the deskew part of the C++17 host mirror (include/icp_mi355x.hpp): a sweep deskewed on its own with explicit
// times and with times from the rows' azimuths (deskew), the twist of a relative pose (deskew_twist), and the odometry
// stream deskewing each raw scan with the twist of its last delta before it filters it (OdometryStream::set_deskew).
// Compiled -fsyntax-only -Wall -Wextra -Werror by tests/test_deskew_header.py.
#include <array>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "icp_mi355x.hpp"

namespace slam = icp_mi355x;

int main()
{
    slam::Context ctx;
    // one ring of a sweep: 360 returns at 10 m, counter-clockwise from -pi, half a step off the seam
    std::vector<double> rows, times;
    for (int k = 0; k < 360; ++k) {
        const double tau = (k + 0.5) / 360.0, az = -3.14159265358979323846 + 6.28318530717958647692 * tau;
        rows.insert(rows.end(), {10.0 * std::cos(az), 10.0 * std::sin(az), -1.0});
        times.push_back(tau);
    }
    const slam::PointCloud sweep(rows);

    static_assert(ICPMI_DESKEW_TIMES == 0 && ICPMI_DESKEW_AZIMUTH == 1, "the C header's time sources");
    static_assert(static_cast<int>(slam::DeskewTimeSource::Azimuth) == ICPMI_DESKEW_AZIMUTH, "the mirror's are the same");
    static_assert(sizeof(icpmi_deskew_config) == 104, "the C struct has no hidden padding");
    static_assert(std::is_same<decltype(slam::DeskewConfig().twist), std::array<double, 6>>::value, "(omega, v)");

    slam::Transformation delta = slam::Transformation::identity();
    slam::DeskewConfig config;
    config.twist = slam::deskew_twist(delta);                 // a standing sensor: six zeros
    config.twist[3] = 1.2;                                    // 1.2 m forward per sweep ...
    config.twist[2] = 0.03;                                   // ... while turning 0.03 rad
    const slam::PointCloud by_time = slam::deskew(ctx, sweep, times, config);
    const slam::PointCloud by_azimuth = slam::deskew(ctx, sweep, config);
    std::printf("%zu rows deskewed with times, %zu with azimuth times\n", by_time.size(), by_azimuth.size());

    slam::OdometryStream stream(&ctx);
    std::array<double, 6> twist{};
    for (int frame = 0; frame < 3; ++frame) {
        config.twist = twist;                                  // the caller owns the gate and the pose: it sets the twist
        stream.set_deskew(config);
        const slam::OdometryStream::Step step = stream.push(sweep, 0.5, 100);
        if (step.registered && step.result.converged && step.result.final_error <= 1.0)
            twist = slam::deskew_twist(step.result.transformation);
        else
            twist = std::array<double, 6>{};
    }
    stream.clear_deskew();
    return 0;
}
