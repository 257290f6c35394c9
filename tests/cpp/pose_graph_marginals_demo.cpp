// Exercises the covariances of the C++17 host mirror's PoseGraph (include/icp_mi355x.hpp): marginalCovariance,
// jointMarginalCovariance, relativeCovariance and closureDistance on a chain of n poses with one loop closure.
// Compiled -fsyntax-only -Wall -Wextra -Werror by tests/test_pose_graph_marginals_header.py; run on the device by
// tests/test_gpu_pose_graph_marginals.py, which builds the same graph through the Python mirror and wants the same bytes.
//
//   pose_graph_marginals_demo in.f64 out.f64
// in.f64: n, then row-major the odometry step (16), the closure 5 -> 65 (16), a proposed edge 10 -> 70 (16) and its
// covariance (36).  out.f64: the marginal of pose 40 (36), the joint of (63, 10) (144), the relative covariance of
// (10, 70) (36) and the proposed edge's d^2.
#include <cstdio>
#include <type_traits>
#include <vector>

#include "icp_mi355x.hpp"

namespace slam = icp_mi355x;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    std::vector<double> in(1 + 3 * 16 + 36);
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
    std::fclose(f);
    const std::size_t n = static_cast<std::size_t>(in[0]);
    std::array<double, 16> m;
    std::copy(in.begin() + 1, in.begin() + 17, m.begin());
    const slam::Transformation step(m);
    std::copy(in.begin() + 17, in.begin() + 33, m.begin());
    const slam::Transformation closure(m);
    std::copy(in.begin() + 33, in.begin() + 49, m.begin());
    const slam::Transformation proposed(m);
    slam::Matrix6 edge;
    std::copy(in.begin() + 49, in.begin() + 85, edge.begin());

    slam::Context ctx;
    slam::PoseGraph graph(slam::PoseGraphConfig(), &ctx);
    graph.addPrior(0, slam::Transformation::identity());
    for (std::size_t k = 0; k + 1 < n; ++k) graph.addOdometryFactor(k, k + 1, step);
    graph.addLoopClosure(5, 65, closure);
    if (!graph.optimize()) return 4;

    const slam::Matrix6 one = graph.marginalCovariance(40);
    static_assert(std::is_same<decltype(graph.jointMarginalCovariance({63, 10})), std::vector<double>>::value,
                  "6q x 6q doubles, row-major");
    const std::vector<double> joint = graph.jointMarginalCovariance({63, 10});
    const slam::Matrix6 rel = graph.relativeCovariance(10, 70);
    const double d2 = graph.closureDistance(10, 70, proposed, edge);
    std::printf("sigma of pose 40: %.3g rad, %.3g m; d2 of the proposed edge %.4g\n", one[0], one[21], d2);

    std::vector<double> out(one.begin(), one.end());
    out.insert(out.end(), joint.begin(), joint.end());
    out.insert(out.end(), rel.begin(), rel.end());
    out.push_back(d2);
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 5;
    std::fclose(f);
    return 0;
}
