// Exercises the loop-edge loss of the C++17 host mirror's PoseGraph (include/icp_mi355x.hpp): the node's back end with a
// robust loss on its loop closures, and the closures the loss refused read back after optimize().  Compiled
// -fsyntax-only -Wall -Wextra -Werror by tests/test_pose_graph_loss_header.py.
#include <cstdio>
#include <type_traits>
#include <utility>
#include <vector>

#include "icp_mi355x.hpp"

namespace slam = icp_mi355x;

int main()
{
    slam::PoseGraph graph;
    graph.setLoopLoss(ICPMI_PG_LOSS_CAUCHY, 1.0);                                   // before or after the factors
    static_assert(std::is_same<decltype(graph.loopLoss()), std::pair<int, double>>::value, "loopLoss: kind, scale");
    static_assert(std::is_same<decltype(graph.loopWeights()),
                               std::pair<std::vector<double>, std::vector<double>>>::value,
                  "loopWeights: weights, distances");
    graph.addPrior(0, slam::Transformation::identity());
    const slam::Transformation step = slam::Transformation::from_rt({1, 0, 0, 0, 1, 0, 0, 0, 1}, {1.0, 0.0, 0.0});
    for (std::size_t k = 1; k <= 20; ++k) graph.addOdometryFactor(k - 1, k, step, 0.01);
    graph.addLoopClosure(0, 20, slam::Transformation::from_rt({1, 0, 0, 0, 1, 0, 0, 0, 1}, {19.9, 0.0, 0.0}));
    graph.addLoopClosure(3, 17, slam::Transformation::identity());                 // two places that only look alike
    const std::pair<int, double> loss = graph.loopLoss();
    std::printf("loss kind=%d scale=%.3f\n", loss.first, loss.second);
    if (graph.optimize()) {
        const auto wd = graph.loopWeights();                                        // in addLoopClosure order
        for (std::size_t e = 0; e < wd.first.size(); ++e)
            std::printf("closure %zu: weight %.3g at %.1f sigmas%s\n", e, wd.first[e], wd.second[e],
                        wd.first[e] < 1e-3 ? " (refused)" : "");
    }
    graph.setLoopLoss(ICPMI_PG_LOSS_NONE);                                          // back to the reference's model
    static_assert(ICPMI_PG_LOSS_HUBER == 1 && ICPMI_PG_LOSS_GEMAN_MCCLURE == 3, "the kinds of icp_mi355x.h");
    return 0;
}
