// pose_graph_info_host.h -- the host half of the pose graph's full-information factors (pose_graph_info.h),
// for host and device compilers alike: no HIP in here.  capi.hip wraps the two functions into the C ABI
// (icpmi_information_from_icp, icpmi_pose_graph_add_*_information) and tests/cpp/pose_graph_info_check.cpp runs them
// with the host compiler.  fp64, every sum in ascending index order, no FMA wanted (capi.hip is built -ffp-contract=off;
// scripts/pose_graph_info_ref.py restates both, operation for operation).
#pragma once
#include <cmath>

namespace icpmi {

// position of R[a][b], a <= b, in the 21 doubles of an upper triangle stored row by row
constexpr int pg_tri(int a, int b) { return 6 * a - a * (a - 1) / 2 + (b - a); }

// Symmetry is asked of |L_ab - L_ba| against sqrt(L_aa L_bb), the natural size of an entry of a positive definite matrix
// (|L_ab| <= sqrt(L_aa L_bb)).  An entry of a 6 x 6 triple product A^T M A is a sum of 36 products of three doubles:
// formed in two orders it differs by at most gamma_38 = 38 * 2^-53 / (1 - ..) ~ 4.2e-15 times the sum of the products'
// magnitudes.  That sum exceeds the entry's natural size by the cancellation in it, which for the lever arms (<= 1e3 m
// against rotations of order 1) and conditions (<= 1e6) of this library's callers stays below 1e5: 4.2e-15 * 1e5 < 1e-9.
// A matrix further from symmetric than that was not rounded into it, it was built wrong.
constexpr double kPgInfoSymTol = 1e-9;

// why a matrix was refused (0: it was not)
enum PgInfoRefusal { kPgInfoOk = 0, kPgInfoNotFinite, kPgInfoAsymmetric, kPgInfoNotPositive };

// Upper Cholesky L = R^T R of a row-major 6 x 6 information matrix (noiseModel::Gaussian::Information keeps this R and
// whitens with it): R's 21 upper entries row by row into R21.  Only the upper triangle of L is factored; the lower one
// is held to it by the symmetry test.  Every pivot must be finite and > 0.  R21 is written only on success.
inline PgInfoRefusal pg_info_cholesky(const double *L, double *R21)
{
    for (int e = 0; e < 36; ++e)
        if (!std::isfinite(L[e])) return kPgInfoNotFinite;
    for (int a = 0; a < 6; ++a)
        if (!(L[6 * a + a] > 0.0)) return kPgInfoNotPositive;
    for (int a = 0; a < 6; ++a)
        for (int b = a + 1; b < 6; ++b)
            if (!(std::fabs(L[6 * a + b] - L[6 * b + a]) <= kPgInfoSymTol * std::sqrt(L[6 * a + a] * L[6 * b + b])))
                return kPgInfoAsymmetric;
    double R[21];
    for (int a = 0; a < 6; ++a) {
        double d = L[6 * a + a];
        for (int k = 0; k < a; ++k) d = d - R[pg_tri(k, a)] * R[pg_tri(k, a)];
        if (!(d > 0.0) || !std::isfinite(d)) return kPgInfoNotPositive;
        const double p = std::sqrt(d);
        R[pg_tri(a, a)] = p;
        for (int b = a + 1; b < 6; ++b) {
            double s = L[6 * a + b];
            for (int k = 0; k < a; ++k) s = s - R[pg_tri(k, a)] * R[pg_tri(k, b)];
            R[pg_tri(a, b)] = s / p;
        }
    }
    for (int e = 0; e < 21; ++e) R21[e] = R[e];
    return kPgInfoOk;
}

// info = Ad_T^T (JtJ / sigma^2) Ad_T + diag(1 / floor_r^2 x 3, 1 / floor_t^2 x 3), Ad_T = [[R, 0], [t^ R, R]] (se3_adjoint's
// ordering).  JtJ: row-major 6 x 6 of which the upper triangle is read; T row-major 4 x 4.  M = JtJ / (sigma sigma) entry
// by entry, P = M Ad, then info_ab = sum_l Ad_la P_lb for a <= b, mirrored: symmetric by construction.  A floor of 0 adds
// nothing.  false: an argument is not finite, sigma is not > 0 or a floor is < 0.
inline bool pg_information_from_icp(const double *JtJ, const double *T, double sigma, double floor_r, double floor_t,
                                    double *info)
{
    if (!std::isfinite(sigma) || !(sigma > 0.0)) return false;
    if (!std::isfinite(floor_r) || !std::isfinite(floor_t) || floor_r < 0.0 || floor_t < 0.0) return false;
    for (int e = 0; e < 36; ++e)
        if (!std::isfinite(JtJ[e])) return false;
    for (int e = 0; e < 16; ++e)
        if (!std::isfinite(T[e])) return false;
    double Ad[36], M[36], P[36];
    const double t[3] = {T[3], T[7], T[11]};
    const double hat[9] = {0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double r = T[4 * i + j];
            Ad[6 * i + j] = r;
            Ad[6 * i + 3 + j] = 0.0;
            Ad[6 * (3 + i) + 3 + j] = r;
            Ad[6 * (3 + i) + j] = (hat[3 * i] * T[j] + hat[3 * i + 1] * T[4 + j]) + hat[3 * i + 2] * T[8 + j];
        }
    const double s2 = sigma * sigma;
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) M[6 * a + b] = JtJ[a <= b ? 6 * a + b : 6 * b + a] / s2;
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
            double s = 0.0;
            for (int l = 0; l < 6; ++l) s = s + M[6 * a + l] * Ad[6 * l + b];
            P[6 * a + b] = s;
        }
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) {
            double s = 0.0;
            for (int l = 0; l < 6; ++l) s = s + Ad[6 * l + a] * P[6 * l + b];
            info[6 * a + b] = s;
            info[6 * b + a] = s;
        }
    for (int a = 0; a < 3; ++a) {
        if (floor_r > 0.0) info[7 * a] = info[7 * a] + 1.0 / (floor_r * floor_r);
        if (floor_t > 0.0) info[7 * (3 + a)] = info[7 * (3 + a)] + 1.0 / (floor_t * floor_t);
    }
    return true;
}

} // namespace icpmi
