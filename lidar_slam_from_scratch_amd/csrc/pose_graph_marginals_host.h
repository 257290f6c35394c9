// pose_graph_marginals_host.h -- the host half of the pose graph's covariances (pose_graph_marginals.h), for
// host and device compilers alike: no HIP in here.  capi.hip wraps the two functions into the C ABI
// (icpmi_pose_graph_relative_covariance, icpmi_pose_graph_closure_distance) and tests/cpp/pose_graph_marginals_check.cpp
// runs them with the host compiler.  fp64, every sum in ascending index order, no FMA wanted (capi.hip is built
// -ffp-contract=off; scripts/pose_graph_marginals_ref.py restates both).
//
// A pose is 12 doubles, R row-major (9) then t (3), as in se3.h, whose maps the few below repeat for the host; the
// tangent order is (omega, v), perturbations on the right: X Exp(xi).
#pragma once
#include <cmath>

namespace icpmi {

inline void pgm_inv(const double *T, double *o)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[3 * i + j] = T[3 * j + i];
    for (int i = 0; i < 3; ++i) o[9 + i] = -((o[3 * i] * T[9] + o[3 * i + 1] * T[10]) + o[3 * i + 2] * T[11]);
}

inline void pgm_mul(const double *a, const double *b, double *o)
{
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
        o[9 + i] = ((a[3 * i] * b[9] + a[3 * i + 1] * b[10]) + a[3 * i + 2] * b[11]) + a[9 + i];
    }
}

// Pose3::AdjointMap in (w, v) order: [R, 0; t^ R, R]
inline void pgm_adjoint(const double *T, double *Ad)
{
    const double *t = T + 9;
    const double hat[9] = {0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            Ad[6 * r + c] = T[3 * r + c];
            Ad[6 * r + c + 3] = 0.0;
            Ad[6 * (r + 3) + c] = (hat[3 * r] * T[c] + hat[3 * r + 1] * T[3 + c]) + hat[3 * r + 2] * T[6 + c];
            Ad[6 * (r + 3) + c + 3] = T[3 * r + c];
        }
}

// Pose3::Logmap as se3_log (se3.h): Rot3::Logmap through the unit quaternion, v = (I - W/2 + D W^2) t
inline void pgm_log(const double *T, double *xi)
{
    const double r00 = T[0], r01 = T[1], r02 = T[2], r10 = T[3], r11 = T[4], r12 = T[5], r20 = T[6], r21 = T[7], r22 = T[8];
    const double tr = r00 + r11 + r22;
    double w, x, y, z;
    if (tr >= r00 && tr >= r11 && tr >= r22) {
        w = 0.5 * std::sqrt(1.0 + tr);
        const double f = 0.25 / w;
        x = (r21 - r12) * f; y = (r02 - r20) * f; z = (r10 - r01) * f;
    } else if (r00 >= r11 && r00 >= r22) {
        x = 0.5 * std::sqrt(1.0 + r00 - r11 - r22);
        const double f = 0.25 / x;
        w = (r21 - r12) * f; y = (r01 + r10) * f; z = (r02 + r20) * f;
    } else if (r11 >= r22) {
        y = 0.5 * std::sqrt(1.0 - r00 + r11 - r22);
        const double f = 0.25 / y;
        w = (r02 - r20) * f; x = (r01 + r10) * f; z = (r12 + r21) * f;
    } else {
        z = 0.5 * std::sqrt(1.0 - r00 - r11 + r22);
        const double f = 0.25 / z;
        w = (r10 - r01) * f; x = (r02 + r20) * f; y = (r12 + r21) * f;
    }
    if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    const double s = std::sqrt(x * x + y * y + z * z);
    double g;
    if (s < 1e-6 * w) {
        const double q = s / w;
        g = 2.0 / w * (1.0 - q * q / 3.0);
    } else {
        g = 2.0 * std::atan2(s, w) / s;
    }
    xi[0] = g * x; xi[1] = g * y; xi[2] = g * z;
    const double th = std::sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]), t2 = th * th;
    double D;
    if (th < 0.1) {
        D = 1.0 / 12 + t2 * (1.0 / 720 + t2 * (1.0 / 30240 + t2 * (1.0 / 1209600 + t2 / 47900160)));
    } else {
        const double h = std::sin(0.5 * th);
        D = 1.0 / (th * th) - std::sin(th) / (4.0 * th * h * h);
    }
    const double W[9] = {0.0, -xi[2], xi[1], xi[2], 0.0, -xi[0], -xi[1], xi[0], 0.0};
    for (int i = 0; i < 3; ++i) {
        double v = 0.0;
        for (int j = 0; j < 3; ++j) {
            const double w2 = (W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j]) + W[3 * i + 2] * W[6 + j];
            v = v + (((i == j) ? 1.0 : 0.0) - 0.5 * W[3 * i + j] + D * w2) * T[9 + j];
        }
        xi[3 + i] = v;
    }
}

// First-order covariance of the tangent of X_i^-1 X_j: with X_i Exp(a), X_j Exp(b) the relative pose moves by
// Exp(-Ad(X_j^-1 X_i) a + b), so Sigma_rel = J Sigma J^T, J = [-Ad(X_j^-1 X_i), I].  joint: 12 x 12 row-major, blocks in
// the order (i, j).  out is symmetric by construction (the upper triangle is formed and mirrored).
inline void pg_relative_covariance(const double *Xi, const double *Xj, const double *joint, double *out)
{
    double Xji[12], inv[12], A[36], J[72], P[72];
    pgm_inv(Xj, inv);
    pgm_mul(inv, Xi, Xji);
    pgm_adjoint(Xji, A);
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
            J[12 * a + b] = -A[6 * a + b];
            J[12 * a + 6 + b] = (a == b) ? 1.0 : 0.0;
        }
    for (int a = 0; a < 6; ++a)          // P = J Sigma (6 x 12)
        for (int b = 0; b < 12; ++b) {
            double s = 0.0;
            for (int l = 0; l < 12; ++l) s = s + J[12 * a + l] * joint[12 * l + b];
            P[12 * a + b] = s;
        }
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) {
            double s = 0.0;
            for (int l = 0; l < 12; ++l) s = s + P[12 * a + l] * J[12 * b + l];
            out[6 * a + b] = s;
            out[6 * b + a] = s;
        }
}

// d^2 = e^T (Sigma_rel + Sigma_edge)^-1 e, e = Log(Z^-1 X_i^-1 X_j): the squared Mahalanobis distance of a proposed edge
// Z against what the graph already says about i and j.  The sum's upper triangle is factored (lower Cholesky of its
// mirror); false where an entry is not finite or a pivot is not > 0.
inline bool pg_closure_distance(const double *Xi, const double *Xj, const double *Z, const double *rel_cov,
                                const double *edge_cov, double *d2)
{
    double inv[12], rel[12], E[12], e[6], M[36], y[6];
    pgm_inv(Xi, inv);
    pgm_mul(inv, Xj, rel);
    pgm_inv(Z, inv);
    pgm_mul(inv, rel, E);
    pgm_log(E, e);
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b <= a; ++b) {
            M[6 * a + b] = rel_cov[6 * b + a] + edge_cov[6 * b + a];
            if (!std::isfinite(M[6 * a + b])) return false;
        }
    for (int j = 0; j < 6; ++j) {
        double d = M[6 * j + j];
        for (int l = 0; l < j; ++l) d = d - M[6 * j + l] * M[6 * j + l];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        const double p = std::sqrt(d);
        M[6 * j + j] = p;
        for (int i = j + 1; i < 6; ++i) {
            double s = M[6 * i + j];
            for (int l = 0; l < j; ++l) s = s - M[6 * i + l] * M[6 * j + l];
            M[6 * i + j] = s / p;
        }
    }
    double sum = 0.0;
    for (int i = 0; i < 6; ++i) {
        double s = e[i];
        for (int l = 0; l < i; ++l) s = s - M[6 * i + l] * y[l];
        y[i] = s / M[6 * i + i];
        sum = sum + y[i] * y[i];
    }
    if (!std::isfinite(sum)) return false;
    *d2 = sum;
    return true;
}

} // namespace icpmi
