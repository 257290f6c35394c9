// deskew.h -- motion compensation of a scan in its sensor frame (not in the reference, which takes every
// scan as a snapshot from one pose).  A spinning sensor measures row i at tau_i in [0, 1] of its sweep while it moves by
// the twist xi = (omega, v) per sweep (se3.h's tangent order, in the sensor frame): pose(tau) = pose(t_ref) Exp((tau -
// t_ref) xi).  k_deskew moves each row into the frame at t_ref:
//     s  = tau_i - t_ref                          tau_i: times[i] as given (ICPMI_DESKEW_TIMES), or from the row's azimuth
//     p' = R(s) p + t(s)                          (ICPMI_DESKEW_AZIMUTH): d = atan2(y, x) - azimuth_start,
//                                                 u = (direction * d) / 2 pi, tau = u - floor(u)
// With theta = |omega|, a = omega / theta, K = hat(a) -- all formed once per sweep on the host (deskew_host.h) and handed
// over by value -- R(s) = I + sin(s theta) K + (1 - cos(s theta)) K^2 and t(s) = s v + ((1 - cos(s theta)) / theta) (a x v)
// + ((s theta - sin(s theta)) / theta) (a x (a x v)).  fp64, unfused, in this order (scripts/deskew_ref.py restates it
// byte for byte; the library's sincos from pi/4 on and atan2 aside):
//     sphi = s * theta;  (sn, cs) = sincos_step(fabs(sphi));  sn = s < 0 ? -sn : sn;  c1 = 1 - cs
//     b = c1 / theta;  cc = (sphi - sn) / theta
//     per coordinate i:  kp  = (K[i][0] x + K[i][1] y) + K[i][2] z
//                        kkp = (K2[i][0] x + K2[i][1] y) + K2[i][2] z
//                        rp  = (p_i + sn * kp) + c1 * kkp
//                        t   = (s * v_i + b * av_i) + cc * aav_i
//                        p'_i = rp + t
//     theta < 1e-10 (twist_to_transform's cut):  p'_i = p_i + s * v_i
// A row with a non-finite coordinate or time, a row with s == 0, and every row under a twist of six zeros pass through
// unchanged in every bit (so -0.0 stays -0.0).  One row per thread with a grid stride, k_transform's launch shape; out may
// alias in (a thread reads its row before it writes it and touches no other).  A wave's three 8-byte loads at a 24-byte
// stride cover 1,536 consecutive bytes between them: every line fetched is used whole.  Bytes per row: 24 read + 24
// written, + 8 with explicit times.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "deskew_host.h"
#include "device_math.h"

namespace icpmi {

constexpr int kDeskewThreads = 256;
constexpr int kDeskewMaxBlocks = 2048; // k_transform's cap: one pass of the grid covers 524,288 rows

// times: n doubles in TIMES mode, not read in AZIMUTH mode (may be null)
__global__ __launch_bounds__(kDeskewThreads) void k_deskew(const double *in, const double *__restrict__ times, double *out, size_t n,
                                                           const DeskewConstants c)
{
    const size_t stride = (size_t)gridDim.x * kDeskewThreads;
    for (size_t i = (size_t)blockIdx.x * kDeskewThreads + threadIdx.x; i < n; i += stride) {
        const double x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
        double tau;
        if (c.time_source == kDeskewTimes) {
            tau = times[i];
        } else {
            const double d = atan2(y, x) - c.azimuth_start;
            const double u = (c.direction * d) / kDeskewTwoPi;
            tau = u - floor(u);
        }
        const double s = tau - c.t_ref;
        double ox = x, oy = y, oz = z;
        if (c.mode != kDeskewIdentity && isfinite(x) && isfinite(y) && isfinite(z) && isfinite(tau) && s != 0.0) {
            if (c.mode == kDeskewTranslation) {
                ox = x + s * c.v[0];
                oy = y + s * c.v[1];
                oz = z + s * c.v[2];
            } else {
                const double sphi = s * c.theta;
                double sn, cs;
                sincos_step(fabs(sphi), &sn, &cs);
                sn = s < 0.0 ? -sn : sn;
                const double c1 = 1.0 - cs;
                const double b = c1 / c.theta, cc = (sphi - sn) / c.theta;
                double o[3];
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const double kp = (c.K[3 * e] * x + c.K[3 * e + 1] * y) + c.K[3 * e + 2] * z;
                    const double kkp = (c.K2[3 * e] * x + c.K2[3 * e + 1] * y) + c.K2[3 * e + 2] * z;
                    const double pe = e == 0 ? x : (e == 1 ? y : z);
                    const double rp = (pe + sn * kp) + c1 * kkp;
                    const double t = (s * c.v[e] + b * c.av[e]) + cc * c.aav[e];
                    o[e] = rp + t;
                }
                ox = o[0], oy = o[1], oz = o[2];
            }
        }
        out[3 * i] = ox, out[3 * i + 1] = oy, out[3 * i + 2] = oz;
    }
}

} // namespace icpmi
