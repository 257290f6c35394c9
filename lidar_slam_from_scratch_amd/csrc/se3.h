// se3.h -- SE(3) maps of the pose-graph back end (pose_graph.h), fp64, one thread per pose or factor.
//
// The same formulas as scripts/pose_graph_ref.py (the CPU restatement the device optimiser is tested against):
// GTSAM 4.x Pose3 with GTSAM_POSE3_EXPMAP / GTSAM_ROT3_EXPMAP, tangent order (omega, v).  A pose is 12 doubles:
// R row-major (9), then t (3).  Matrices are row-major.
#pragma once
#include <hip/hip_runtime.h>

namespace icpmi {

constexpr double kSe3Small = 0.1;   // series forms of the cancelling coefficients below this angle
constexpr double kSe3Tiny = 1e-8;   // series forms of sin(t)/t and (1 - cos t)/t^2 below this angle

struct Se3Coefs {
    double A, B, C, D, E, F;
};

// A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3, D = 1/t^2 - (1 + cos t) / (2 t sin t),
// E = (t^2 + 2 cos t - 2) / (2 t^4), F = (2 t - 3 sin t + t cos t) / (2 t^5)
__device__ inline Se3Coefs se3_coefs(double th)
{
    Se3Coefs k;
    const double t2 = th * th;
    if (th < kSe3Tiny) {
        k.A = 1.0 - t2 / 6.0;
        k.B = 0.5 - t2 / 24.0;
    } else {
        const double h = sin(0.5 * th);
        k.A = sin(th) / th;
        k.B = 2.0 * h * h / (th * th);
    }
    if (th < kSe3Small) {
        k.C = 1.0 / 6 - t2 * (1.0 / 120 - t2 * (1.0 / 5040 - t2 * (1.0 / 362880 - t2 / 39916800)));
        k.D = 1.0 / 12 + t2 * (1.0 / 720 + t2 * (1.0 / 30240 + t2 * (1.0 / 1209600 + t2 / 47900160)));
        k.E = 1.0 / 24 - t2 * (1.0 / 720 - t2 * (1.0 / 40320 - t2 * (1.0 / 3628800 - t2 / 479001600)));
        k.F = 1.0 / 120 - t2 * (1.0 / 2520 - t2 * (1.0 / 120960 - t2 * (1.0 / 9979200 - t2 / 1245404160)));
    } else {
        const double s = sin(th), c = cos(th), h = sin(0.5 * th);
        const double t4 = (th * th) * (th * th);
        k.C = (th - s) / (th * th * th);
        k.D = 1.0 / (th * th) - s / (4.0 * th * h * h);
        k.E = (th * th + 2.0 * c - 2.0) / (2.0 * t4);
        k.F = (2.0 * th - 3.0 * s + th * c) / (2.0 * (t4 * th));
    }
    return k;
}

__device__ inline void m3_mul(const double *a, const double *b, double *o)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
__device__ inline void m3_hat(const double *w, double *W)
{
    W[0] = 0.0;   W[1] = -w[2]; W[2] = w[1];
    W[3] = w[2];  W[4] = 0.0;   W[5] = -w[0];
    W[6] = -w[1]; W[7] = w[0];  W[8] = 0.0;
}
__device__ inline void m3_vec(const double *a, const double *v, double *o)
{
    for (int i = 0; i < 3; ++i) o[i] = a[3 * i] * v[0] + a[3 * i + 1] * v[1] + a[3 * i + 2] * v[2];
}

// Pose3::Expmap: R = I + A W + B W^2, t = (I + B W + C W^2) v
__device__ inline void se3_exp(const double *xi, double *T)
{
    double W[9], W2[9];
    m3_hat(xi, W);
    m3_mul(W, W, W2);
    const double th = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
    const Se3Coefs k = se3_coefs(th);
    double V[9];
    for (int e = 0; e < 9; ++e) {
        const double I = (e % 4 == 0) ? 1.0 : 0.0;
        T[e] = I + k.A * W[e] + k.B * W2[e];
        V[e] = I + k.B * W[e] + k.C * W2[e];
    }
    m3_vec(V, xi + 3, T + 9);
}

// Rot3::Logmap through the unit quaternion (Shepperd: the largest component first), w >= 0
__device__ inline void so3_log(const double *R, double *w_out)
{
    const double r00 = R[0], r01 = R[1], r02 = R[2], r10 = R[3], r11 = R[4], r12 = R[5], r20 = R[6], r21 = R[7], r22 = R[8];
    const double tr = r00 + r11 + r22;
    double w, x, y, z;
    if (tr >= r00 && tr >= r11 && tr >= r22) {
        w = 0.5 * sqrt(1.0 + tr);
        const double f = 0.25 / w;
        x = (r21 - r12) * f; y = (r02 - r20) * f; z = (r10 - r01) * f;
    } else if (r00 >= r11 && r00 >= r22) {
        x = 0.5 * sqrt(1.0 + r00 - r11 - r22);
        const double f = 0.25 / x;
        w = (r21 - r12) * f; y = (r01 + r10) * f; z = (r02 + r20) * f;
    } else if (r11 >= r22) {
        y = 0.5 * sqrt(1.0 - r00 + r11 - r22);
        const double f = 0.25 / y;
        w = (r02 - r20) * f; x = (r01 + r10) * f; z = (r12 + r21) * f;
    } else {
        z = 0.5 * sqrt(1.0 - r00 - r11 + r22);
        const double f = 0.25 / z;
        w = (r10 - r01) * f; x = (r02 + r20) * f; y = (r12 + r21) * f;
    }
    if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    const double s = sqrt(x * x + y * y + z * z);
    double g;
    if (s < 1e-6 * w) {
        const double q = s / w;
        g = 2.0 / w * (1.0 - q * q / 3.0);
    } else {
        g = 2.0 * atan2(s, w) / s;
    }
    w_out[0] = g * x; w_out[1] = g * y; w_out[2] = g * z;
}

// Pose3::Logmap: w = Log(R), v = (I - W/2 + D W^2) t
__device__ inline void se3_log(const double *T, double *xi)
{
    so3_log(T, xi);
    double W[9], W2[9];
    m3_hat(xi, W);
    m3_mul(W, W, W2);
    const double th = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
    const double D = se3_coefs(th).D;
    double Vi[9];
    for (int e = 0; e < 9; ++e) Vi[e] = ((e % 4 == 0) ? 1.0 : 0.0) - 0.5 * W[e] + D * W2[e];
    m3_vec(Vi, T + 9, xi + 3);
}

// Pose3::LogmapDerivative: [Jw^-1, 0; -Jw^-1 Q Jw^-1, Jw^-1], Jw^-1 = I + W/2 + D W^2,
// Q = -V/2 + C (WV + VW - WVW) - E (WWV + VWW - 3 WVW) + F (WVWW + WWVW)
__device__ inline void se3_jr_inv(const double *xi, double *J /* 36 */)
{
    double W[9], V[9], WW[9], WV[9], VW[9], WVW[9], t1[9], t2[9], t3[9], t4[9];
    m3_hat(xi, W);
    m3_hat(xi + 3, V);
    const double th = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
    const Se3Coefs k = se3_coefs(th);
    m3_mul(W, W, WW);
    m3_mul(W, V, WV);
    m3_mul(V, W, VW);
    m3_mul(WV, W, WVW);
    m3_mul(WW, V, t1);    // WWV
    m3_mul(VW, W, t2);    // VWW
    m3_mul(WVW, W, t3);   // WVWW
    m3_mul(WW, VW, t4);   // WWVW
    double Q[9], Ji[9];
    for (int e = 0; e < 9; ++e) {
        Q[e] = -0.5 * V[e] + k.C * (WV[e] + VW[e] - WVW[e]) - k.E * (t1[e] + t2[e] - 3.0 * WVW[e]) + k.F * (t3[e] + t4[e]);
        Ji[e] = ((e % 4 == 0) ? 1.0 : 0.0) + 0.5 * W[e] + k.D * WW[e];
    }
    double JQ[9], JQJ[9];
    m3_mul(Ji, Q, JQ);
    m3_mul(JQ, Ji, JQJ);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            J[6 * r + c] = Ji[3 * r + c];
            J[6 * r + c + 3] = 0.0;
            J[6 * (r + 3) + c] = -JQJ[3 * r + c];
            J[6 * (r + 3) + c + 3] = Ji[3 * r + c];
        }
}

// Pose3::inverse: (R^T, -(R^T t))
__device__ inline void se3_inv(const double *T, double *o)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[3 * i + j] = T[3 * j + i];
    double v[3];
    m3_vec(o, T + 9, v);
    o[9] = -v[0]; o[10] = -v[1]; o[11] = -v[2];
}
// Pose3::compose: (Ra Rb, Ra tb + ta)
__device__ inline void se3_mul(const double *a, const double *b, double *o)
{
    m3_mul(a, b, o);
    double v[3];
    m3_vec(a, b + 9, v);
    o[9] = v[0] + a[9]; o[10] = v[1] + a[10]; o[11] = v[2] + a[11];
}
// Pose3::AdjointMap in (w, v) order: [R, 0; t^ R, R]
__device__ inline void se3_adjoint(const double *T, double *Ad)
{
    double th[9], tR[9];
    m3_hat(T + 9, th);
    m3_mul(th, T, tR);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            Ad[6 * r + c] = T[3 * r + c];
            Ad[6 * r + c + 3] = 0.0;
            Ad[6 * (r + 3) + c] = tR[3 * r + c];
            Ad[6 * (r + 3) + c + 3] = T[3 * r + c];
        }
}

} // namespace icpmi
