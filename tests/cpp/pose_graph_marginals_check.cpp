// Host check of csrc/pose_graph_marginals_host.h, the host half of the pose graph's covariances: the relative covariance
// of two poses on cases with a known answer, every refusal of pg_closure_distance (what icpmi_pose_graph_closure_distance
// returns ICPMI_ERR_ARG for), and, with arguments, the two functions as a filter for
// tests/test_pose_graph_marginals_host.py: doubles in as hex floats, doubles out as hex floats.  Built with the host
// compiler; no GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "pose_graph_marginals_host.h"

using namespace icpmi;

static int failures = 0;
#define EXPECT(cond)                                                                                                    \
    do {                                                                                                                \
        if (!(cond)) {                                                                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);                                                       \
            ++failures;                                                                                                 \
        }                                                                                                               \
    } while (0)

static void to12(const double *T, double *o)   // row-major 4 x 4 -> R (9), t (3)
{
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o[3 * r + c] = T[4 * r + c];
        o[9 + r] = T[4 * r + 3];
    }
}

static int filter(int argc, char **argv)
{
    // rel Xi[16] Xj[16] joint[144] -> 36 doubles | dist Xi[16] Xj[16] Z[16] rel_cov[36] edge_cov[36] -> ok, then d2
    static double in[256];
    const int n = argc - 2;
    for (int i = 0; i < n && i < 256; ++i) in[i] = std::strtod(argv[2 + i], nullptr);
    double Xi[12], Xj[12], Z[12];
    if (!std::strcmp(argv[1], "rel") && n == 176) {
        double out[36];
        to12(in, Xi);
        to12(in + 16, Xj);
        pg_relative_covariance(Xi, Xj, in + 32, out);
        for (int e = 0; e < 36; ++e) std::printf("%a\n", out[e]);
        return 0;
    }
    if (!std::strcmp(argv[1], "dist") && n == 120) {
        double d2 = 0.0;
        to12(in, Xi);
        to12(in + 16, Xj);
        to12(in + 32, Z);
        const bool ok = pg_closure_distance(Xi, Xj, Z, in + 48, in + 84, &d2);
        std::printf("%d\n%a\n", ok ? 1 : 0, d2);
        return 0;
    }
    return 2;
}

int main(int argc, char **argv)
{
    if (argc > 1) return filter(argc, argv);
    const double I12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    double joint[144], out[36], eye[36], d2 = -1.0;
    for (int e = 0; e < 36; ++e) eye[e] = e % 7 == 0 ? 1.0 : 0.0;

    // two poses at the identity: Sigma_rel = S_ii - S_ij - S_ji + S_jj
    for (int a = 0; a < 12; ++a)
        for (int b = 0; b < 12; ++b) joint[12 * a + b] = (a == b ? 2.0 : 0.0) + ((a % 6 == b % 6) ? 0.5 : 0.0);
    pg_relative_covariance(I12, I12, joint, out);
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) EXPECT(out[6 * a + b] == (a == b ? 4.0 : 0.0));   // 2.5 - 0.5 - 0.5 + 2.5

    // j = i moved 3 m along x, joint = [S S Ad^T; Ad S, Ad S Ad^T + Q] (i's covariance carried to j plus Q): Sigma_rel = Q
    double Xj[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 3, 0, 0}, inv[12], Ad[36];
    pgm_inv(Xj, inv);
    pgm_adjoint(inv, Ad);                        // Ad(X_j^-1 X_i) with X_i = I
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
            double ad_adt = 0.0;
            for (int l = 0; l < 6; ++l) ad_adt += Ad[6 * a + l] * Ad[6 * b + l];
            joint[12 * a + b] = eye[6 * a + b];
            joint[12 * a + 6 + b] = Ad[6 * b + a];
            joint[12 * (6 + a) + b] = Ad[6 * a + b];
            joint[12 * (6 + a) + 6 + b] = ad_adt + (a == b ? 0.25 : 0.0);
        }
    pg_relative_covariance(I12, Xj, joint, out);
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) EXPECT(std::fabs(out[6 * a + b] - (a == b ? 0.25 : 0.0)) <= 1e-14);

    // a proposed edge that is exactly the relative pose: e = 0, d2 = 0
    EXPECT(pg_closure_distance(I12, Xj, Xj, eye, eye, &d2) && d2 == 0.0);
    // off by 1 m along x under a total covariance of 2 I: d2 = 0.5
    const double Z[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 2, 0, 0};
    EXPECT(pg_closure_distance(I12, Xj, Z, eye, eye, &d2) && std::fabs(d2 - 0.5) <= 1e-15);

    // refusals: a sum that is not positive definite, or not finite; d2 is left alone
    double bad[36];
    d2 = -7.0;
    for (int e = 0; e < 36; ++e) bad[e] = -eye[e];
    EXPECT(!pg_closure_distance(I12, Xj, Z, eye, bad, &d2));                      // the sum is zero
    for (int e = 0; e < 36; ++e) bad[e] = -2.0 * eye[e];
    EXPECT(!pg_closure_distance(I12, Xj, Z, eye, bad, &d2));                      // negative definite
    std::memcpy(bad, eye, sizeof(bad));
    bad[1] = bad[6] = 3.0;
    EXPECT(!pg_closure_distance(I12, Xj, Z, eye, bad, &d2));                      // indefinite
    std::memcpy(bad, eye, sizeof(bad));
    bad[14] = std::numeric_limits<double>::quiet_NaN();
    EXPECT(!pg_closure_distance(I12, Xj, Z, eye, bad, &d2));
    bad[14] = std::numeric_limits<double>::infinity();
    EXPECT(!pg_closure_distance(I12, Xj, Z, eye, bad, &d2));
    EXPECT(d2 == -7.0);

    if (failures) return 1;
    std::printf("ok pose_graph_marginals_host\n");
    return 0;
}
