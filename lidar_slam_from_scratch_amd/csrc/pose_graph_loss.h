// pose_graph_loss.h -- a robust loss on the pose graph's loop-closure edges: GTSAM 4.1+ noiseModel::Robust over the loop
// factors' diagonal model, restated from the source as published (scripts/pose_graph_loss_ref.py is the CPU
// restatement; there is no GTSAM build to check against).
//
// The setting is the graph's, not a factor's: it applies to every factor added by add_loop_closure, past and future, at
// the next optimize().  Priors and odometry factors are never touched.  Per loop factor rw = r / sigma and
// d = sqrt(sum rw_a^2), `scale` k in whitened units (sigmas):
//     ICPMI_PG_LOSS_HUBER (1)          w = d <= k ? 1 : k / d              rho = d <= k ? 0.5 d^2 : k (d - 0.5 k)
//     ICPMI_PG_LOSS_CAUCHY (2)         s = k k,  w = s / (s + d^2)         rho = 0.5 s log1p(d^2 / s)
//     ICPMI_PG_LOSS_GEMAN_MCCLURE (3)  s = k k,  q = s / (s + d^2), w = q q   rho = 0.5 s d^2 / (s + d^2)
// No form divides by d except Huber's outer branch, where d > k > 0.
// Linearisation (Robust::WhitenSystem): A_i, A_j and rw of a loop factor are multiplied by sqrt(w) (q itself for
// Geman-McClure, sqrt() for the other two); H, g and the linearised error are formed from the scaled values.
// Error (NoiseModelFactor::error -> Robust::loss): a loop factor contributes rho(d), every other factor 0.5 d^2, for the
// initial error, every trial's candidate error, the history and final_error.  The LM policy is untouched.
//
//   k_pg_linearize_loss  k_pg_linearize with the scaling above; lin.err[f] = rho, and each factor's linearised error at
//                        a zero step, 0.5 ||sqrt(w) rw||^2 (under a loss no longer the error itself)
//   k_pg_trial_loss      k_pg_trial with rho for the candidate error; the linearised half reads the scaled lin.A / lin.rw
//   k_pg_loop_weights    one thread per factor over the optimised values: (w, d) of a loop factor to its rank among the
//                        loop factors
//
// PgFactor.reserved carries "is a loop closure" (1 from icpmi_pose_graph_add_loop_closure, 0 elsewhere); the kernels of
// pose_graph.h ignore the field, and are what runs while the loss is off or the graph has no loop factor.  fp64 and
// fixed-order sums throughout, so repeated optimize() calls under a loss stay bit-identical.
#pragma once
#include "pose_graph.h"

namespace icpmi {

constexpr int kPgLossNone = 0, kPgLossHuber = 1, kPgLossCauchy = 2, kPgLossGemanMcClure = 3;

// weight, sqrt(weight) and loss of whitened distance d (d2 = d d) under loss `kind` of scale k
__device__ inline void pg_loss(int kind, double k, double d2, double &w, double &sw, double &rho)
{
    if (kind == kPgLossHuber) {
        const double d = sqrt(d2);
        if (d <= k) {
            w = 1.0;
            sw = 1.0;
            rho = 0.5 * d2;
        } else {
            w = k / d;
            sw = sqrt(w);
            rho = k * (d - 0.5 * k);
        }
    } else if (kind == kPgLossCauchy) {
        const double s = k * k;
        w = s / (s + d2);
        sw = sqrt(w);
        rho = 0.5 * s * log1p(d2 / s);
    } else if (kind == kPgLossGemanMcClure) {
        const double s = k * k, q = s / (s + d2);
        w = q * q;
        sw = q;
        rho = 0.5 * s * d2 / (s + d2);
    } else {
        w = 1.0;
        sw = 1.0;
        rho = 0.5 * d2;
    }
}

__global__ void k_pg_linearize_loss(const PgFactor *__restrict__ fac, const int32_t *__restrict__ map, int F,
                                    const double *__restrict__ X, PgLin lin, int loss, double scale,
                                    double *__restrict__ err_lin0)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const PgFactor fa = fac[f];
    double r[6], Ji[36], Jj[36];
    pg_residual(fa, map, X, r, Ji, Jj);
    double rw[6], e = 0.0;
    for (int a = 0; a < 6; ++a) {
        rw[a] = r[a] * fa.inv_sigma[a];
        e = e + rw[a] * rw[a];
    }
    double w = 1.0, sw = 1.0, rho = 0.5 * e;
    const bool loop = fa.reserved == 1;
    if (loop) pg_loss(loss, scale, e, w, sw, rho);
    double e0 = 0.0;
    for (int a = 0; a < 6; ++a) {
        const double is = fa.inv_sigma[a];
        for (int b = 0; b < 6; ++b) {
            double ji = Ji[6 * a + b] * is;
            double jj = fa.kind == 1 ? Jj[6 * a + b] * is : 0.0;
            if (loop) {
                ji = ji * sw;
                jj = jj * sw;
            }
            Ji[6 * a + b] = ji;
            Jj[6 * a + b] = jj;
        }
        if (loop) rw[a] = rw[a] * sw;
        e0 = e0 + rw[a] * rw[a];
    }
    lin.err[f] = rho;
    err_lin0[f] = 0.5 * e0;
    double *A = lin.A + 72 * (size_t)f, *H = lin.H + 108 * (size_t)f, *g = lin.g + 12 * (size_t)f;
    for (int a = 0; a < 6; ++a) lin.rw[6 * (size_t)f + a] = rw[a];
    for (int q = 0; q < 36; ++q) {
        A[q] = Ji[q];
        A[36 + q] = Jj[q];
    }
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
            double hii = 0.0, hjj = 0.0, hij = 0.0;
            for (int l = 0; l < 6; ++l) {
                hii = hii + Ji[6 * l + a] * Ji[6 * l + b];
                hjj = hjj + Jj[6 * l + a] * Jj[6 * l + b];
                hij = hij + Ji[6 * l + a] * Jj[6 * l + b];
            }
            H[6 * a + b] = hii;
            H[36 + 6 * a + b] = hjj;
            H[72 + 6 * a + b] = hij;
        }
    for (int a = 0; a < 6; ++a) {
        double gi = 0.0, gj = 0.0;
        for (int l = 0; l < 6; ++l) {
            gi = gi + Ji[6 * l + a] * rw[l];
            gj = gj + Jj[6 * l + a] * rw[l];
        }
        g[a] = gi;
        g[6 + a] = gj;
    }
}

// per factor: error at the candidate values (rho for a loop factor), and the linearised error
// 0.5 ||A_i d_i + A_j d_j + rw||^2 of the already scaled lin.A / lin.rw
__global__ void k_pg_trial_loss(const PgFactor *__restrict__ fac, const int32_t *__restrict__ map, int F,
                                const double *__restrict__ Xc, const PgLin lin, const double *__restrict__ delta,
                                int loss, double scale, double *__restrict__ err_c, double *__restrict__ err_lin)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const PgFactor fa = fac[f];
    double r[6];
    pg_residual(fa, map, Xc, r, nullptr, nullptr);
    double e = 0.0, el = 0.0;
    const double *A = lin.A + 72 * (size_t)f;
    const double *di = delta + 6 * (size_t)map[fa.i];
    const double *dj = fa.kind == 1 ? delta + 6 * (size_t)map[fa.j] : nullptr;
    for (int a = 0; a < 6; ++a) {
        const double w = r[a] * fa.inv_sigma[a];
        e = e + w * w;
        double s = 0.0;
        for (int l = 0; l < 6; ++l) s = s + A[6 * a + l] * di[l];
        if (dj) {
            double s2 = 0.0;
            for (int l = 0; l < 6; ++l) s2 = s2 + A[36 + 6 * a + l] * dj[l];
            s = s + s2;
        }
        s = s + lin.rw[6 * (size_t)f + a];
        el = el + s * s;
    }
    double w = 1.0, sw = 1.0, rho = 0.5 * e;
    if (fa.reserved == 1) pg_loss(loss, scale, e, w, sw, rho);
    err_c[f] = rho;
    err_lin[f] = 0.5 * el;
}

// rank[f] = position of loop factor f among the loop factors (add_loop_closure order), -1 for every other factor;
// wd[2 rank] = w, wd[2 rank + 1] = d at values X.  loss 0: w = 1.
__global__ void k_pg_loop_weights(const PgFactor *__restrict__ fac, const int32_t *__restrict__ map,
                                  const int32_t *__restrict__ rank, int F, const double *__restrict__ X, int loss,
                                  double scale, double *__restrict__ wd)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int k = rank[f];
    if (k < 0) return;
    const PgFactor fa = fac[f];
    double r[6];
    pg_residual(fa, map, X, r, nullptr, nullptr);
    double e = 0.0;
    for (int a = 0; a < 6; ++a) {
        const double x = r[a] * fa.inv_sigma[a];
        e = e + x * x;
    }
    double w, sw, rho;
    pg_loss(loss, scale, e, w, sw, rho);
    wd[2 * (size_t)k] = w;
    wd[2 * (size_t)k + 1] = sqrt(e);
}

} // namespace icpmi
