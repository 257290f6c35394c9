// pose_graph_info.h -- between factors weighted by a full 6 x 6 information matrix: GTSAM's
// noiseModel::Gaussian::Information, which keeps the upper Cholesky factor R of L = R^T R and whitens with it,
// rw = R r, A = R J.  scripts/pose_graph_info_ref.py is the CPU restatement.
//
// An information factor is a PgFactor like any other (its inv_sigma is not read) plus a slot: slot[f] >= 0 names 21
// doubles in `Rs`, R's upper triangle row by row (pg_tri, pose_graph_info_host.h), -1 says "diagonal, whiten by
// inv_sigma".  The host factors L when the edge is added (pg_info_cholesky) and refuses what does not factor, so the
// kernels meet only valid R.
//
//   k_pg_linearize_info  k_pg_linearize / k_pg_linearize_loss for a graph that holds an information factor.  A diagonal
//                        factor takes exactly their arithmetic (with the loss off sqrt(w) is 1.0 and a product by it is
//                        exact), so it gives their bits.  R is upper triangular: row a of R x reads rows >= a of x only,
//                        so r and both Jacobians are whitened in place in ascending a, with R read row by row.
//   k_pg_trial_info      k_pg_trial / k_pg_trial_loss with the same whitening
//   k_pg_loop_weights_info   k_pg_loop_weights with d = ||R r|| for an information loop factor
//
// The loop loss of pose_graph_loss.h applies to loop factors of either kind, on d^2 = ||R r||^2.  They run only while the
// graph holds at least one information factor; otherwise the kernels of pose_graph.h / pose_graph_loss.h run, untouched.
// fp64 and fixed-order sums (ascending index), no atomics: repeated optimize() calls stay bit-identical.
#pragma once
#include "pose_graph_info_host.h"
#include "pose_graph_loss.h"

namespace icpmi {

// x (6 rows of `cols` doubles, row stride `cols`) <- R x, in place; R21 in global memory, one row at a time
__device__ inline void pg_whiten_rows(const double *__restrict__ R21, double *x, int cols)
{
    for (int a = 0; a < 6; ++a) {
        double row[6];
        for (int l = a; l < 6; ++l) row[l] = R21[pg_tri(a, l)];
        for (int b = 0; b < cols; ++b) {
            double s = 0.0;
            for (int l = a; l < 6; ++l) s = s + row[l] * x[cols * l + b];
            x[cols * a + b] = s;
        }
    }
}

constexpr int kPgInfoThreads = 128;   // k_pg_linearize_info's workgroup (capi.hip launches it with this)

// err_lin0 may be null (loss off: the linearised error at a zero step is the error itself).
// Launch bounds: r, both Jacobians and what se3_jr_inv / se3_adjoint hold are ~130 doubles per thread; under the
// default bound of 1024 threads the compiler has 128 VGPRs and spills (as k_pg_linearize and k_pg_linearize_loss do),
// under 128 threads it has 512.
__global__ __launch_bounds__(kPgInfoThreads) void k_pg_linearize_info(
    const PgFactor *__restrict__ fac, const int32_t *__restrict__ slot, const double *__restrict__ Rs,
    const int32_t *__restrict__ map, int F, const double *__restrict__ X, PgLin lin, int loss, double scale,
    double *__restrict__ err_lin0)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const PgFactor fa = fac[f];
    const int sl = slot[f];
    double r[6], Ji[36], Jj[36];
    pg_residual(fa, map, X, r, Ji, Jj);
    double rw[6], e = 0.0;
    if (sl >= 0) {
        const double *R21 = Rs + 21 * (size_t)sl;
        for (int a = 0; a < 6; ++a) rw[a] = r[a];
        pg_whiten_rows(R21, rw, 1);
        pg_whiten_rows(R21, Ji, 6);
        if (fa.kind == 1) pg_whiten_rows(R21, Jj, 6);
        for (int a = 0; a < 6; ++a) e = e + rw[a] * rw[a];
    } else {
        for (int a = 0; a < 6; ++a) {
            rw[a] = r[a] * fa.inv_sigma[a];
            e = e + rw[a] * rw[a];
        }
    }
    double w = 1.0, sw = 1.0, rho = 0.5 * e;
    const bool loop = fa.reserved == 1;
    if (loop) pg_loss(loss, scale, e, w, sw, rho);
    double e0 = 0.0;
    for (int a = 0; a < 6; ++a) {
        const double is = sl >= 0 ? 1.0 : fa.inv_sigma[a];
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
    if (err_lin0) err_lin0[f] = 0.5 * e0;
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

// squared whitened distance of residual r: ||R r||^2 for an information factor, sum (r_a / sigma_a)^2 otherwise
__device__ inline double pg_whitened_d2(const PgFactor &fa, int sl, const double *__restrict__ Rs, const double *r)
{
    double e = 0.0;
    if (sl >= 0) {
        const double *R21 = Rs + 21 * (size_t)sl;
        for (int a = 0; a < 6; ++a) {
            double s = 0.0;
            for (int l = a; l < 6; ++l) s = s + R21[pg_tri(a, l)] * r[l];
            e = e + s * s;
        }
    } else {
        for (int a = 0; a < 6; ++a) {
            const double w = r[a] * fa.inv_sigma[a];
            e = e + w * w;
        }
    }
    return e;
}

__global__ void k_pg_trial_info(const PgFactor *__restrict__ fac, const int32_t *__restrict__ slot,
                                const double *__restrict__ Rs, const int32_t *__restrict__ map, int F,
                                const double *__restrict__ Xc, const PgLin lin, const double *__restrict__ delta,
                                int loss, double scale, double *__restrict__ err_c, double *__restrict__ err_lin)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const PgFactor fa = fac[f];
    double r[6];
    pg_residual(fa, map, Xc, r, nullptr, nullptr);
    const double e = pg_whitened_d2(fa, slot[f], Rs, r);
    double el = 0.0;
    const double *A = lin.A + 72 * (size_t)f;
    const double *di = delta + 6 * (size_t)map[fa.i];
    const double *dj = fa.kind == 1 ? delta + 6 * (size_t)map[fa.j] : nullptr;
    for (int a = 0; a < 6; ++a) {
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

__global__ void k_pg_loop_weights_info(const PgFactor *__restrict__ fac, const int32_t *__restrict__ slot,
                                       const double *__restrict__ Rs, const int32_t *__restrict__ map,
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
    const double e = pg_whitened_d2(fa, slot[f], Rs, r);
    double w, sw, rho;
    pg_loss(loss, scale, e, w, sw, rho);
    wd[2 * (size_t)k] = w;
    wd[2 * (size_t)k + 1] = sqrt(e);
}

} // namespace icpmi
