// Host check of csrc/deskew_host.h, the host half of the motion compensation: every refusal of
// deskew_check, the per-sweep constants' three forms, and the log map's round trips and refusals.  A stand-alone program;
// tests/test_deskew_header.py builds it with the host compiler under -fsanitize=address,undefined and runs it.
//     deskew_host_check                   the checks; prints "ok <n> checks"
//     deskew_host_check twist <16 hex>    deskew_twist of a row-major 4 x 4 -> 6 hex doubles (or "refused")
//     deskew_host_check consts <6 hex>    deskew_constants of a twist -> mode, theta, K, K2, av, aav as hex doubles
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "deskew_host.h"

using namespace icpmi;

static int g_checks = 0;
#define CHECK(cond)                                                                           \
    do {                                                                                      \
        ++g_checks;                                                                           \
        if (!(cond)) {                                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                     \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

// Exp(xi) as a row-major 4 x 4 (se3.h's se3_exp; C's series below 0.1 rad is cut after t^6: its next term is below 1e-16)
static void exp_se3(const double xi[6], double T[16])
{
    const double th = std::sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
    const double W[9] = {0.0, -xi[2], xi[1], xi[2], 0.0, -xi[0], -xi[1], xi[0], 0.0};
    double W2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W2[3 * i + j] = W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j];
    double A = 1.0, B = 0.5, C = 1.0 / 6;
    if (th > 0.0) {
        A = std::sin(th) / th;
        B = 2.0 * std::sin(0.5 * th) * std::sin(0.5 * th) / (th * th);
        const double t2 = th * th;
        C = th < 0.1 ? 1.0 / 6 - t2 / 120 + t2 * t2 / 5040 - t2 * t2 * t2 / 362880 : (th - std::sin(th)) / (th * th * th);
    }
    for (int e = 0; e < 16; ++e) T[e] = e == 15 ? 1.0 : 0.0;
    for (int i = 0; i < 3; ++i) {
        double t = 0.0;
        for (int j = 0; j < 3; ++j) {
            const double I = i == j ? 1.0 : 0.0;
            T[4 * i + j] = I + A * W[3 * i + j] + B * W2[3 * i + j];
            t += (I + B * W[3 * i + j] + C * W2[3 * i + j]) * xi[3 + j];
        }
        T[4 * i + 3] = t;
    }
}

static int run_checks()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double pi = 3.14159265358979323846;
    double tw[6] = {0.01, -0.02, 0.03, 1.0, 0.2, -0.1};
    // ---- deskew_check: every refusal, in the order the header states
    CHECK(deskew_check(tw, 0.5, kDeskewTimes, 1, -pi) == kDeskewOk);
    CHECK(deskew_check(tw, 0.0, kDeskewAzimuth, -1, 0.3) == kDeskewOk);
    CHECK(deskew_check(tw, 1.0, kDeskewAzimuth, 1, 100.0) == kDeskewOk);
    for (int e = 0; e < 6; ++e)
        for (double bad : {nan, inf, -inf}) {
            double b[6];
            std::memcpy(b, tw, sizeof(b));
            b[e] = bad;
            CHECK(deskew_check(b, 0.5, kDeskewTimes, 1, -pi) == kDeskewTwistNotFinite);
        }
    for (double bad : {nan, inf, -inf}) {
        CHECK(deskew_check(tw, bad, kDeskewTimes, 1, -pi) == kDeskewTRefNotFinite);
        CHECK(deskew_check(tw, 0.5, kDeskewTimes, 1, bad) == kDeskewAzimuthNotFinite);
    }
    CHECK(deskew_check(tw, -1e-300, kDeskewTimes, 1, -pi) == kDeskewTRefRange);
    CHECK(deskew_check(tw, std::nextafter(1.0, 2.0), kDeskewTimes, 1, -pi) == kDeskewTRefRange);
    for (int bad : {0, 2, -2, 1 << 30})
        CHECK(deskew_check(tw, 0.5, kDeskewTimes, bad, -pi) == kDeskewDirection);
    for (int bad : {-1, 2, 77})
        CHECK(deskew_check(tw, 0.5, bad, 1, -pi) == kDeskewTimeSource);
    for (int r = kDeskewOk; r <= kDeskewTimeSource; ++r)
        CHECK((std::strlen(deskew_refusal_text((DeskewRefusal)r)) > 0) == (r != kDeskewOk));
    // the first failing rule is the one reported
    {
        double b[6] = {nan, 0, 0, 0, 0, 0};
        CHECK(deskew_check(b, 7.0, 9, 0, nan) == kDeskewTwistNotFinite);
        CHECK(deskew_check(tw, 7.0, 9, 0, -pi) == kDeskewTRefRange);
        CHECK(deskew_check(tw, 0.5, 9, 0, -pi) == kDeskewDirection);
    }
    // ---- deskew_constants: the three forms
    {
        const double zero[6] = {0, 0, 0, 0, 0, 0}, negzero[6] = {-0.0, 0, 0, 0, -0.0, 0};
        CHECK(deskew_constants(zero, 0.5, kDeskewTimes, 1, -pi).mode == kDeskewIdentity);
        CHECK(deskew_constants(negzero, 0.5, kDeskewTimes, 1, -pi).mode == kDeskewIdentity);
        const double slide[6] = {0, 0, 0, 1.5, 0, 0}, tiny[6] = {3e-11, -4e-11, 0, 1.5, 0, 0}, edge[6] = {1e-10, 0, 0, 0, 0, 0};
        CHECK(deskew_constants(slide, 0.5, kDeskewTimes, 1, -pi).mode == kDeskewTranslation);
        DeskewConstants c = deskew_constants(tiny, 0.5, kDeskewTimes, 1, -pi);
        CHECK(c.mode == kDeskewTranslation && std::fabs(c.theta - 5e-11) < 1e-25 && c.v[0] == 1.5);
        for (int e = 0; e < 9; ++e) CHECK(c.K[e] == 0.0 && c.K2[e] == 0.0);
        CHECK(deskew_constants(edge, 0.5, kDeskewTimes, 1, -pi).mode == kDeskewFull);   // the cut is theta < 1e-10
        const double yaw[6] = {0, 0, 0.25, 2.0, 3.0, 4.0};
        c = deskew_constants(yaw, 0.25, kDeskewAzimuth, -1, 0.5);
        CHECK(c.mode == kDeskewFull && c.theta == 0.25 && c.direction == -1.0 && c.t_ref == 0.25 && c.azimuth_start == 0.5);
        CHECK(c.time_source == kDeskewAzimuth);
        const double K[9] = {0, -1, 0, 1, 0, 0, 0, 0, 0}, K2[9] = {-1, 0, 0, 0, -1, 0, 0, 0, 0};
        for (int e = 0; e < 9; ++e) CHECK(c.K[e] == K[e] && c.K2[e] == K2[e]);
        CHECK(c.av[0] == -3.0 && c.av[1] == 2.0 && c.av[2] == 0.0);       // z x v
        CHECK(c.aav[0] == -2.0 && c.aav[1] == -3.0 && c.aav[2] == 0.0);   // z x (z x v)
    }
    // ---- deskew_twist: round trips Log(Exp(xi)) == xi, the identity, and the refusals
    {
        double T[16], out[6];
        const double zero[6] = {0, 0, 0, 0, 0, 0};
        exp_se3(zero, T);
        CHECK(deskew_twist(T, out));
        for (int e = 0; e < 6; ++e) CHECK(out[e] == 0.0);
        const double cases[][6] = {{1e-3, 0, 0, 1, 0, 0},         {0, -2e-3, 1e-3, 0.3, 2, -1}, {0.01, 0.02, -0.03, 1.2, 0.1, 0.0},
                                   {0.05, -0.04, 0.06, -2, 1, 0.5}, {0.3, -0.2, 0.4, 1, 2, 3},     {0, 0, 0.7, 2, 0, 0},
                                   {1.0, 1.0, -1.0, 0.5, -0.5, 2}, {0, 0, 0, 1.5, -0.25, 0.125},  {0, 3.0, 0, 1, 1, 1}};
        for (const auto &xi : cases) {
            exp_se3(xi, T);
            CHECK(deskew_twist(T, out));
            for (int e = 0; e < 6; ++e) CHECK(std::fabs(out[e] - xi[e]) <= 1e-14 * (1.0 + std::fabs(xi[e]))); // ~30 roundings of entries <= 3
        }
        // the last row is not read; any non-finite entry of the upper 3 x 4 is refused and nothing is written
        exp_se3(cases[2], T);
        T[12] = nan, T[15] = inf;
        CHECK(deskew_twist(T, out));
        for (int e = 0; e < 12; ++e)
            for (double bad : {nan, inf}) {
                double B[16], o[6] = {7, 7, 7, 7, 7, 7};
                exp_se3(cases[2], B);
                B[e] = bad;
                CHECK(!deskew_twist(B, o));
                for (int q = 0; q < 6; ++q) CHECK(o[q] == 7.0);
            }
    }
    std::printf("ok %d checks\n", g_checks);
    return 0;
}

static double from_hex(const char *s) { return std::strtod(s, nullptr); }

int main(int argc, char **argv)
{
    if (argc == 1) return run_checks();
    if (argc == 18 && !std::strcmp(argv[1], "twist")) {
        double T[16], out[6];
        for (int e = 0; e < 16; ++e) T[e] = from_hex(argv[2 + e]);
        if (!deskew_twist(T, out)) {
            std::printf("refused\n");
            return 0;
        }
        for (int e = 0; e < 6; ++e) std::printf("%a ", out[e]);
        std::printf("\n");
        return 0;
    }
    if (argc == 8 && !std::strcmp(argv[1], "consts")) {
        double tw[6];
        for (int e = 0; e < 6; ++e) tw[e] = from_hex(argv[2 + e]);
        const DeskewConstants c = deskew_constants(tw, 0.5, kDeskewTimes, 1, 0.0);
        std::printf("%d %a ", c.mode, c.theta);
        for (int e = 0; e < 9; ++e) std::printf("%a ", c.K[e]);
        for (int e = 0; e < 9; ++e) std::printf("%a ", c.K2[e]);
        for (int e = 0; e < 3; ++e) std::printf("%a ", c.av[e]);
        for (int e = 0; e < 3; ++e) std::printf("%a ", c.aav[e]);
        std::printf("\n");
        return 0;
    }
    std::printf("usage: deskew_host_check [twist <16 hex doubles> | consts <6 hex doubles>]\n");
    return 2;
}
