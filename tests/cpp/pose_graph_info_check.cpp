// Host check of csrc/pose_graph_info_host.h, the host half of the pose graph's information factors: every refusal of
// pg_information_from_icp (what icpmi_information_from_icp returns ICPMI_ERR_ARG for) and of pg_info_cholesky (what
// icpmi_pose_graph_add_*_information return ICPMI_ERR_ARG for), R^T R = info on what it accepts, and, with arguments, the
// two functions as a filter for tests/test_pose_graph_info_host.py: doubles in as hex floats, doubles out as hex floats,
// so that the Python restatement can be held to the same bits.  Built with the host compiler; no GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "pose_graph_info_host.h"

using namespace icpmi;

static int failures = 0;
#define EXPECT(cond)                                                                                                    \
    do {                                                                                                                \
        if (!(cond)) {                                                                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);                                                       \
            ++failures;                                                                                                 \
        }                                                                                                               \
    } while (0)

static void identity(double *T)
{
    for (int e = 0; e < 16; ++e) T[e] = e % 5 == 0 ? 1.0 : 0.0;
}

static int filter(int argc, char **argv)
{
    // info JtJ[36] T[16] sigma floor_r floor_t -> 36 doubles | chol info[36] -> refusal code, then 21 doubles
    double in[64];
    const int n = argc - 2;
    for (int i = 0; i < n && i < 64; ++i) in[i] = std::strtod(argv[2 + i], nullptr);
    if (!std::strcmp(argv[1], "info") && n == 55) {
        double out[36];
        if (!pg_information_from_icp(in, in + 36, in[52], in[53], in[54], out)) return 3;
        for (int e = 0; e < 36; ++e) std::printf("%a\n", out[e]);
        return 0;
    }
    if (!std::strcmp(argv[1], "chol") && n == 36) {
        double R[21];
        const int why = pg_info_cholesky(in, R);
        std::printf("%d\n", why);
        if (why == kPgInfoOk)
            for (int e = 0; e < 21; ++e) std::printf("%a\n", R[e]);
        return 0;
    }
    return 2;
}

int main(int argc, char **argv)
{
    if (argc > 1) return filter(argc, argv);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    double J[36] = {0.0}, T[16], out[36];
    identity(T);
    for (int a = 0; a < 6; ++a) J[7 * a] = 4.0 + a;
    J[1] = J[6] = 0.5;
    // ---- pg_information_from_icp: the argument refusals
    EXPECT(pg_information_from_icp(J, T, 0.02, 0.0, 0.0, out));
    EXPECT(pg_information_from_icp(J, T, 0.02, 0.1, 1.0, out));
    for (double sigma : {0.0, -0.02, nan, inf, -inf}) EXPECT(!pg_information_from_icp(J, T, sigma, 0.0, 0.0, out));
    for (double fl : {-1.0, nan, inf, -inf}) {
        EXPECT(!pg_information_from_icp(J, T, 0.02, fl, 0.0, out));
        EXPECT(!pg_information_from_icp(J, T, 0.02, 0.0, fl, out));
    }
    for (double bad : {nan, inf}) {
        double Jb[36], Tb[16];
        std::memcpy(Jb, J, sizeof(J));
        std::memcpy(Tb, T, sizeof(T));
        Jb[8] = bad;
        Tb[7] = bad;
        EXPECT(!pg_information_from_icp(Jb, T, 0.02, 0.0, 0.0, out));
        EXPECT(!pg_information_from_icp(J, Tb, 0.02, 0.0, 0.0, out));
    }
    // identity T, sigma 0.5: info = 4 JtJ exactly, symmetric, the lower triangle of JtJ never read
    J[6] = 99.0;
    EXPECT(pg_information_from_icp(J, T, 0.5, 0.0, 0.0, out));
    EXPECT(out[1] == 2.0 && out[6] == 2.0 && out[0] == 16.0 && out[35] == 36.0);
    J[6] = 0.5;
    // the floors land on the diagonal: 1 / 0.5^2 = 4 on the rotations, 1 / 0.25^2 = 16 on the translations
    EXPECT(pg_information_from_icp(J, T, 0.5, 0.5, 0.25, out));
    EXPECT(out[0] == 20.0 && out[14] == 28.0 && out[21] == 44.0 && out[35] == 52.0 && out[1] == 2.0);

    // ---- pg_info_cholesky: the refusals of icpmi_pose_graph_add_*_information
    double R[21], L[36];
    for (int e = 0; e < 21; ++e) R[e] = -7.0;
    auto refused = [&](PgInfoRefusal why) {
        const PgInfoRefusal got = pg_info_cholesky(L, R);
        bool untouched = true;
        for (int e = 0; e < 21; ++e) untouched = untouched && R[e] == -7.0;
        return got == why && untouched;
    };
    EXPECT(pg_information_from_icp(J, T, 0.5, 0.0, 0.0, L));
    double keep[36];
    std::memcpy(keep, L, sizeof(L));
    L[9] = nan;
    EXPECT(refused(kPgInfoNotFinite));
    L[9] = inf;
    EXPECT(refused(kPgInfoNotFinite));
    std::memcpy(L, keep, sizeof(L));
    L[1] = L[1] + 1e-3;                                   // asymmetric: 1e-3 of an entry of size 2 against diagonals of 16, 20
    EXPECT(refused(kPgInfoAsymmetric));
    std::memcpy(L, keep, sizeof(L));
    L[1] = L[1] * (1.0 + 1e-13);                          // what rounding leaves is not: accepted
    EXPECT(pg_info_cholesky(L, R) == kPgInfoOk);
    for (int e = 0; e < 21; ++e) R[e] = -7.0;
    std::memcpy(L, keep, sizeof(L));
    L[1] = L[6] = 100.0;                                  // indefinite: |L01| > sqrt(L00 L11)
    EXPECT(refused(kPgInfoNotPositive));
    std::memcpy(L, keep, sizeof(L));
    L[14] = -L[14];                                       // a negative diagonal entry
    EXPECT(refused(kPgInfoNotPositive));
    // semi-definite without a floor: one plane z = 0 seen at integer points, J rows [y, -x, 0, 0, 0, 1] -- exact in fp64,
    // rank 3, every pivot of the null directions exactly 0
    double P[36] = {0.0};
    for (int x = -2; x <= 2; ++x)
        for (int y = -2; y <= 2; ++y) {
            const double j[6] = {(double)y, (double)-x, 0.0, 0.0, 0.0, 1.0};
            for (int a = 0; a < 6; ++a)
                for (int b = 0; b < 6; ++b) P[6 * a + b] += j[a] * j[b];
        }
    EXPECT(pg_information_from_icp(P, T, 1.0, 0.0, 0.0, L));
    EXPECT(refused(kPgInfoNotPositive));
    EXPECT(pg_information_from_icp(P, T, 1.0, 1.0, 10.0, L));   // ... and with a floor it factors
    EXPECT(pg_info_cholesky(L, R) == kPgInfoOk);
    // R^T R = info on a full matrix
    double Tm[16];
    identity(Tm);
    Tm[0] = 0.0; Tm[1] = -1.0; Tm[4] = 1.0; Tm[5] = 0.0;   // Rz(90 deg)
    Tm[3] = 3.0; Tm[7] = -2.0; Tm[11] = 0.5;
    EXPECT(pg_information_from_icp(J, Tm, 0.02, 0.0, 0.0, L));
    EXPECT(pg_info_cholesky(L, R) == kPgInfoOk);
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) {
            double s = 0.0;
            for (int k = 0; k <= a; ++k) s += R[pg_tri(k, a)] * R[pg_tri(k, b)];
            EXPECT(std::fabs(s - L[6 * a + b]) <= 1e-12 * std::sqrt(L[7 * a] * L[7 * b]));
            EXPECT(L[6 * a + b] == L[6 * b + a]);
        }
    for (int a = 0; a < 6; ++a) EXPECT(R[pg_tri(a, a)] > 0.0);
    if (failures) return 1;
    std::printf("ok pose_graph_info_host\n");
    return 0;
}
