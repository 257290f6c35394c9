// deskew_host.h -- the host half of the motion compensation of a scan (deskew.h), for host and device
// compilers alike: no HIP in here.  capi.hip wraps these into the C ABI (icpmi_deskew*, icpmi_deskew_twist,
// icpmi_stream_set_deskew) and tests/cpp/deskew_host_check.cpp runs them with the host compiler.  fp64, every sum in the
// order written, no FMA wanted (capi.hip is built -ffp-contract=off; scripts/deskew_ref.py restates all three, operation
// for operation):
//     deskew_check       why a configuration is refused
//     deskew_constants   what k_deskew is handed by value: formed once per sweep, never per row
//     deskew_twist       the SE(3) log of a relative pose (se3.h's se3_log: the same formulas and small-angle forms)
#pragma once
#include <cmath>
#include <stdint.h>

namespace icpmi {

constexpr int kDeskewTimes = 0, kDeskewAzimuth = 1;                        // ICPMI_DESKEW_TIMES, ICPMI_DESKEW_AZIMUTH
constexpr int kDeskewIdentity = 0, kDeskewTranslation = 1, kDeskewFull = 2; // DeskewConstants::mode
constexpr double kDeskewTinyAngle = 1e-10;                                 // twist_to_transform's cut
constexpr double kDeskewTwoPi = 6.28318530717958647692;

// why a configuration was refused (0: it was not)
enum DeskewRefusal { kDeskewOk = 0, kDeskewTwistNotFinite, kDeskewTRefNotFinite, kDeskewAzimuthNotFinite, kDeskewTRefRange,
                     kDeskewDirection, kDeskewTimeSource };

inline const char *deskew_refusal_text(DeskewRefusal r)
{
    switch (r) {
    case kDeskewOk: return "";
    case kDeskewTwistNotFinite: return "a deskew twist entry is not finite";
    case kDeskewTRefNotFinite: return "the deskew t_ref is not finite";
    case kDeskewAzimuthNotFinite: return "the deskew azimuth_start is not finite";
    case kDeskewTRefRange: return "the deskew t_ref must lie in [0, 1]";
    case kDeskewDirection: return "the deskew direction must be +1 or -1";
    default: return "unknown deskew time_source";
    }
}

inline DeskewRefusal deskew_check(const double twist[6], double t_ref, int32_t time_source, int32_t direction, double azimuth_start)
{
    for (int e = 0; e < 6; ++e)
        if (!std::isfinite(twist[e])) return kDeskewTwistNotFinite;
    if (!std::isfinite(t_ref)) return kDeskewTRefNotFinite;
    if (!std::isfinite(azimuth_start)) return kDeskewAzimuthNotFinite;
    if (!(t_ref >= 0.0 && t_ref <= 1.0)) return kDeskewTRefRange;
    if (direction != 1 && direction != -1) return kDeskewDirection;
    if (time_source != kDeskewTimes && time_source != kDeskewAzimuth) return kDeskewTimeSource;
    return kDeskewOk;
}

// With theta = |omega|, a = omega / theta, K = hat(a): K, K2 = K K, av = a x v, aav = a x (a x v).  mode: IDENTITY for a
// twist of six zeros (every row passes through in every bit), TRANSLATION below the tiny angle (R = I, t = s v), else
// FULL.  Outside FULL the rotation's constants are zero and unused.
struct DeskewConstants {
    double theta;
    double K[9], K2[9];
    double v[3], av[3], aav[3];
    double t_ref, azimuth_start, direction; // direction: +-1.0
    int32_t mode, time_source;
};

inline DeskewConstants deskew_constants(const double twist[6], double t_ref, int32_t time_source, int32_t direction,
                                        double azimuth_start)
{
    DeskewConstants c{};
    const double wx = twist[0], wy = twist[1], wz = twist[2], vx = twist[3], vy = twist[4], vz = twist[5];
    c.theta = std::sqrt((wx * wx + wy * wy) + wz * wz);
    c.v[0] = vx, c.v[1] = vy, c.v[2] = vz;
    c.t_ref = t_ref, c.azimuth_start = azimuth_start, c.direction = (double)direction;
    c.time_source = time_source;
    if (wx == 0.0 && wy == 0.0 && wz == 0.0 && vx == 0.0 && vy == 0.0 && vz == 0.0) {
        c.mode = kDeskewIdentity;
    } else if (c.theta < kDeskewTinyAngle) {
        c.mode = kDeskewTranslation;
    } else {
        c.mode = kDeskewFull;
        const double ax = wx / c.theta, ay = wy / c.theta, az = wz / c.theta;
        const double K[9] = {0.0, -az, ay, az, 0.0, -ax, -ay, ax, 0.0};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                c.K[3 * i + j] = K[3 * i + j];
                c.K2[3 * i + j] = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
            }
        c.av[0] = ay * vz - az * vy, c.av[1] = az * vx - ax * vz, c.av[2] = ax * vy - ay * vx;
        c.aav[0] = ay * c.av[2] - az * c.av[1], c.aav[1] = az * c.av[0] - ax * c.av[2], c.aav[2] = ax * c.av[1] - ay * c.av[0];
    }
    return c;
}

// twist = Log(delta), delta a row-major 4 x 4 rigid transform (its last row is not read): omega through the unit
// quaternion (Shepperd: the largest component first, w >= 0), v = (I - W/2 + D W^2) t with D's series below 0.1 rad --
// se3.h's so3_log / se3_log / se3_coefs, line for line.  false: an entry of the upper 3 x 4 is not finite (nothing written).
inline bool deskew_twist(const double delta[16], double twist[6])
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j)
            if (!std::isfinite(delta[4 * i + j])) return false;
    const double r00 = delta[0], r01 = delta[1], r02 = delta[2], r10 = delta[4], r11 = delta[5], r12 = delta[6], r20 = delta[8],
                 r21 = delta[9], r22 = delta[10];
    const double t[3] = {delta[3], delta[7], delta[11]};
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
    const double om[3] = {g * x, g * y, g * z};
    const double W[9] = {0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0};
    double W2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W2[3 * i + j] = W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j];
    const double th = std::sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double t2 = th * th;
    double D;
    if (th < 0.1) {
        D = 1.0 / 12 + t2 * (1.0 / 720 + t2 * (1.0 / 30240 + t2 * (1.0 / 1209600 + t2 / 47900160)));
    } else {
        const double sn = std::sin(th), h = std::sin(0.5 * th);
        D = 1.0 / (th * th) - sn / (4.0 * th * h * h);
    }
    double Vi[9];
    for (int e = 0; e < 9; ++e) Vi[e] = ((e % 4 == 0) ? 1.0 : 0.0) - 0.5 * W[e] + D * W2[e];
    for (int i = 0; i < 3; ++i) {
        twist[i] = om[i];
        twist[3 + i] = Vi[3 * i] * t[0] + Vi[3 * i + 1] * t[1] + Vi[3 * i + 2] * t[2];
    }
    return true;
}

} // namespace icpmi
