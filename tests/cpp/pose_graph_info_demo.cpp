// Exercises the information edges of the C++17 host mirror (include/icp_mi355x.hpp): a registration's normal matrix read
// back (last_normal_matrix), turned into the information of its pose-graph edge (information_from_icp) and entered with
// PoseGraph::addOdometryInformation / addLoopClosureInformation; the loop detector attaching the same matrix to its
// results.  Compiled -fsyntax-only -Wall -Wextra -Werror by tests/test_pose_graph_info_header.py.
#include <cstdio>
#include <type_traits>
#include <vector>

#include "icp_mi355x.hpp"

namespace slam = icp_mi355x;

int main()
{
    slam::Context ctx;
    slam::PoseGraph graph(slam::PoseGraphConfig(), &ctx);
    graph.addPrior(0, slam::Transformation::identity());

    std::vector<double> xyz(3 * 2000, 0.0);
    for (std::size_t i = 0; i < 2000; ++i) xyz[3 * i] = 0.01 * static_cast<double>(i), xyz[3 * i + 1] = static_cast<double>(i % 40);
    const slam::ICPResult r = slam::icp_point_to_plane(ctx, xyz.data(), 2000, xyz.data(), 2000);
    const slam::NormalMatrix nm = slam::last_normal_matrix(ctx);               // of the pass that produced final_error
    static_assert(std::is_same<decltype(slam::NormalMatrix::JtJ), slam::Matrix6>::value, "JtJ: 36 doubles, row-major");
    std::printf("pairs %lld, rms %.3g = sqrt(%.3g / %.3g)\n", nm.pairs, r.final_error, nm.sum_sq, nm.weight);

    // sigma: 2 cm of residual noise per pair; the floors keep a single plane's JtJ positive definite
    const slam::Matrix6 info = slam::information_from_icp(nm.JtJ, nm.T, 0.02, 1.0, 10.0);
    graph.addOdometryInformation(0, 1, r.transformation, info);               // from = the target's pose, to = the source's
    graph.addOdometryFactor(1, 2, r.transformation, r.final_error);           // diagonal and information factors mix
    graph.addLoopClosureInformation(0, 2, slam::Transformation::identity(), info);
    graph.setLoopLoss(ICPMI_PG_LOSS_CAUCHY, 1.0);                             // d = ||R r|| for an information loop edge
    if (graph.optimize()) {
        const auto wd = graph.loopWeights();
        std::printf("closure weight %.3g at %.1f sigmas\n", wd.first[0], wd.second[0]);
    }

    slam::LoopClosureConfig lc;
    lc.information_sigma = 0.02;
    lc.information_floor_rotation = 1.0;
    lc.information_floor_translation = 10.0;
    slam::LoopClosureDetector detector(lc, &ctx);
    for (const slam::LoopClosureResult &c : detector.detect())
        if (c.has_information)
            graph.addLoopClosureInformation(static_cast<std::size_t>(c.match_frame), static_cast<std::size_t>(c.query_frame),
                                            c.transform, c.information);
    return 0;
}
