// pose_graph.h -- the pose-graph back end on the GPU: one Levenberg-Marquardt iteration of the reference's GTSAM
// optimiser (core/pose_graph.cpp:147-171) as a handful of plain launches.  The host (capi.hip,
// icpmi_pose_graph_optimize) keeps the LM policy; everything it solves stays in HBM.
//
//   k_pg_gather          initial estimates (by pose index) -> the working values (compact order)
//   k_pg_linearize       one thread per factor: whitened residual, both whitened 6x6 Jacobians, H blocks ii / jj / ij,
//                        g blocks, error
//   k_pg_assemble        per node and entry: diagonal block, gradient and chain coupling H(v, v+1) summed over its
//                        incident factors in factor order (host-built CSR; no atomics)
//   k_pg_segment         one workgroup per segment (a run of non-separator nodes): block Cholesky along the run with
//                        13 right-hand sides (the 12 columns coupling it to its two separators and -g), leaving
//                        Y = A_ss^-1 [A_sB | -g_s] per node and the 12 x 13 Schur contribution to its separators
//   k_pg_reduced         the separators' dense system: lower blocks, and its right-hand side
//   k_chol_diag / _panel / _update   blocked right-looking fp64 Cholesky of it (panel width kCholNb)
//   k_trsv_pair          forward + backward substitution in one workgroup
//   k_pg_backsub         delta of every node: separators from the dense solve, segments delta = Y[:,12] - Y[:,:12] d_B
//   k_pg_retract         candidate X Exp(delta)
//   k_pg_trial           the candidate's factor errors, and each factor's 0.5 ||A delta + r||^2
//   k_pg_reduce          sums of one or two per-factor arrays in a fixed order -> 2 doubles
//
// Every sum runs in an order fixed by the graph alone, so repeated optimize() calls are bit-identical.
#pragma once
#include <hip/hip_runtime.h>
#include "se3.h"

namespace icpmi {

constexpr int kPgChainK = 64;       // every K-th pose index is a separator: segments hold at most K - 1 nodes
constexpr int kCholNb = 32;         // panel width of the reduced Cholesky
constexpr int kPgSegThreads = 192;  // waves 0-1: the 6x6 blocks and the 13 columns; 64..141: the 78 RHS entries

struct PgFactor {
    int32_t kind;                   // 0 prior, 1 between
    int32_t i, j;                   // pose indices (j unused for a prior)
    int32_t reserved;
    double Z[12];                   // measurement: R row-major, t
    double inv_sigma[6];
};

// per-factor linearisation, struct of arrays of stride F
struct PgLin {
    double *A;      // F x 72: A_i (36) then A_j (36), whitened, row-major
    double *rw;     // F x 6: whitened residual
    double *err;    // F: 0.5 ||rw||^2
    double *H;      // F x 108: H_ii, H_jj, H_ij = A_i^T A_j
    double *g;      // F x 12: A_i^T rw, A_j^T rw
};

__global__ void k_pg_gather(const double *__restrict__ init_raw, const int32_t *__restrict__ keys, int n,
                            double *__restrict__ X)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 12) return;
    X[t] = init_raw[12 * (size_t)keys[t / 12] + t % 12];
}

// residual and unwhitened Jacobians of factor f at values X (compact); Jj untouched for a prior
__device__ inline void pg_residual(const PgFactor &fa, const int32_t *map, const double *X, double *r, double *Ji,
                                   double *Jj)
{
    const double *Xi = X + 12 * (size_t)map[fa.i];
    double rel[12], Zi[12], E[12];
    if (fa.kind == 1) {
        double Xinv[12];
        se3_inv(Xi, Xinv);
        se3_mul(Xinv, X + 12 * (size_t)map[fa.j], rel);   // X_i^-1 X_j
    } else {
        for (int e = 0; e < 12; ++e) rel[e] = Xi[e];      // P^-1 X
    }
    se3_inv(fa.Z, Zi);
    se3_mul(Zi, rel, E);
    se3_log(E, r);
    if (!Ji) return;
    double Jr[36];
    se3_jr_inv(r, Jr);
    if (fa.kind == 1) {
        double relinv[12], Ad[36];
        se3_inv(rel, relinv);
        se3_adjoint(relinv, Ad);
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b < 6; ++b) {
                double s = 0.0;
                for (int l = 0; l < 6; ++l) s = s + Jr[6 * a + l] * Ad[6 * l + b];
                Ji[6 * a + b] = -s;
                Jj[6 * a + b] = Jr[6 * a + b];
            }
    } else {
        for (int e = 0; e < 36; ++e) Ji[e] = Jr[e];
    }
}

__global__ void k_pg_linearize(const PgFactor *__restrict__ fac, const int32_t *__restrict__ map, int F,
                               const double *__restrict__ X, PgLin lin)
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
        for (int b = 0; b < 6; ++b) {
            Ji[6 * a + b] = Ji[6 * a + b] * fa.inv_sigma[a];
            Jj[6 * a + b] = fa.kind == 1 ? Jj[6 * a + b] * fa.inv_sigma[a] : 0.0;
        }
    }
    lin.err[f] = 0.5 * e;
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

// node v, entry q in [0, 78): q < 36 diagonal block D_v, q < 42 gradient g_v, else chain coupling Cn_v = H(v, v+1).
// inc[inc_ptr[v] ..] = 2 f + role (role 0: v is the factor's i, 1: its j), ascending f; cn[cn_ptr[v] ..] = chain
// factors (v, v+1), ascending.
__global__ void k_pg_assemble(const PgLin lin, const int32_t *__restrict__ inc_ptr, const int32_t *__restrict__ inc,
                              const int32_t *__restrict__ cn_ptr, const int32_t *__restrict__ cn, int n,
                              double *__restrict__ D, double *__restrict__ g, double *__restrict__ Cn)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 78) return;
    const int v = t / 78, q = t % 78;
    double s = 0.0;
    if (q < 42) {
        for (int p = inc_ptr[v]; p < inc_ptr[v + 1]; ++p) {
            const int f = inc[p] >> 1, role = inc[p] & 1;
            s = s + (q < 36 ? lin.H[108 * (size_t)f + 36 * role + q] : lin.g[12 * (size_t)f + 6 * role + (q - 36)]);
        }
        if (q < 36) D[36 * (size_t)v + q] = s;
        else g[6 * (size_t)v + q - 36] = s;
    } else {
        for (int p = cn_ptr[v]; p < cn_ptr[v + 1]; ++p) s = s + lin.H[108 * (size_t)cn[p] + 72 + (q - 42)];
        Cn[36 * (size_t)v + q - 42] = s;
    }
}

// in-place 6x6 Cholesky (lower) of M; false on a non-positive or non-finite pivot
__device__ inline bool chol6(double *M)
{
    for (int j = 0; j < 6; ++j) {
        double d = M[6 * j + j];
        for (int l = 0; l < j; ++l) d = d - M[6 * j + l] * M[6 * j + l];
        if (!(d > 0.0) || !isfinite(d)) return false;
        const double p = sqrt(d);
        M[6 * j + j] = p;
        for (int i = j + 1; i < 6; ++i) {
            double s = M[6 * i + j];
            for (int l = 0; l < j; ++l) s = s - M[6 * i + l] * M[6 * j + l];
            M[6 * i + j] = s / p;
        }
    }
    for (int i = 0; i < 6; ++i)
        for (int j = i + 1; j < 6; ++j) M[6 * i + j] = 0.0;
    return true;
}

struct PgSeg {
    int32_t start, len, left, right;   // compact nodes start..start+len-1; left / right separator (compact) or -1
};

// Block Cholesky of one segment's block-tridiagonal matrix (diag D_k + lam I, coupling Cn_k) with 13 right-hand
// sides: columns 0-5 couple the first node to the left separator (Cn_L^T), 6-11 the last node to the right one
// (Cn_last), 12 is -g.  Forward: M_k = D_k + lam I - U_{k-1}^T U_{k-1} = L_k L_k^T, U_k = L_k^-1 Cn_k,
// V_k = L_k^-1 (RHS_k - U_{k-1}^T V_{k-1}); backward: Y_k = L_k^-T (V_k - U_k Y_{k+1}).  Schur rows: Cn_L Y_0 (left
// separator) and Cn_last^T Y_last (right one).
__global__ __launch_bounds__(kPgSegThreads) void k_pg_segment(const PgSeg *__restrict__ segs, double lam,
                                                              const double *__restrict__ D, const double *__restrict__ g,
                                                              const double *__restrict__ Cn, double *__restrict__ Lg,
                                                              double *__restrict__ Ug, double *__restrict__ Yg,
                                                              double *__restrict__ schur, int *__restrict__ status)
{
    __shared__ double M[36], Up[36], Vp[78], W[78];
    const PgSeg sg = segs[blockIdx.x];
    const int t = threadIdx.x;
    for (int k = 0; k < sg.len; ++k) {
        const int v = sg.start + k;
        if (t < 36) {
            const int r = t / 6, c = t % 6;
            double s = D[36 * (size_t)v + t] + (r == c ? lam : 0.0);
            if (k > 0) {
                double u = 0.0;
                for (int l = 0; l < 6; ++l) u = u + Up[6 * l + r] * Up[6 * l + c];
                s = s - u;
            }
            M[t] = s;
        } else if (t >= 64 && t < 64 + 78) {
            const int q = t - 64, r = q / 13, c = q % 13;
            double s = 0.0;
            if (c < 6) s = (k == 0 && sg.left >= 0) ? Cn[36 * (size_t)sg.left + 6 * c + r] : 0.0;
            else if (c < 12) s = (k == sg.len - 1 && sg.right >= 0) ? Cn[36 * (size_t)v + 6 * r + (c - 6)] : 0.0;
            else s = -g[6 * (size_t)v + r];
            if (k > 0) {
                double u = 0.0;
                for (int l = 0; l < 6; ++l) u = u + Up[6 * l + r] * Vp[13 * l + c];
                s = s - u;
            }
            W[q] = s;
        }
        __syncthreads();
        if (t == 0 && !chol6(M)) *status = 1;
        __syncthreads();
        if (t < 36) Lg[36 * (size_t)v + t] = M[t];
        if (t >= 64 && t < 64 + 13) {   // V column c = L^-1 W column c
            const int c = t - 64;
            double x[6];
            for (int i = 0; i < 6; ++i) {
                double s = W[13 * i + c];
                for (int l = 0; l < i; ++l) s = s - M[6 * i + l] * x[l];
                x[i] = s / M[6 * i + i];
            }
            for (int i = 0; i < 6; ++i) {
                Vp[13 * i + c] = x[i];
                Yg[78 * (size_t)v + 13 * i + c] = x[i];
            }
        } else if (t >= 96 && t < 102) {   // U column c = L^-1 Cn_v column c (last node: no coupling inside)
            const int c = t - 96;
            double x[6];
            for (int i = 0; i < 6; ++i) {
                double s = (k < sg.len - 1) ? Cn[36 * (size_t)v + 6 * i + c] : 0.0;
                for (int l = 0; l < i; ++l) s = s - M[6 * i + l] * x[l];
                x[i] = s / M[6 * i + i];
            }
            for (int i = 0; i < 6; ++i) {
                Up[6 * i + c] = x[i];
                Ug[36 * (size_t)v + 6 * i + c] = x[i];
            }
        }
        __syncthreads();
    }
    // backward, one thread per column (a column of Y depends only on the same column of the next node's Y)
    if (t < 13) {
        const int c = t;
        double ynext[6] = {0, 0, 0, 0, 0, 0};
        for (int k = sg.len - 1; k >= 0; --k) {
            const int v = sg.start + k;
            const double *L = Lg + 36 * (size_t)v, *U = Ug + 36 * (size_t)v;
            double s[6];
            for (int i = 0; i < 6; ++i) {
                s[i] = Yg[78 * (size_t)v + 13 * i + c];
                if (k < sg.len - 1) {
                    double u = 0.0;
                    for (int l = 0; l < 6; ++l) u = u + U[6 * i + l] * ynext[l];
                    s[i] = s[i] - u;
                }
            }
            for (int i = 5; i >= 0; --i) {
                double a = s[i];
                for (int l = i + 1; l < 6; ++l) a = a - L[6 * l + i] * ynext[l];
                ynext[i] = a / L[6 * i + i];
            }
            // ynext now holds Y_k (the loop above reads only entries it has already replaced)
            for (int i = 0; i < 6; ++i) Yg[78 * (size_t)v + 13 * i + c] = ynext[i];
        }
    }
    __syncthreads();
    if (t < 13) {
        const int c = t;
        double *S = schur + 156 * (size_t)blockIdx.x;
        const int first = sg.start, last = sg.start + sg.len - 1;
        for (int r = 0; r < 6; ++r) {
            double a = 0.0, b = 0.0;
            for (int l = 0; l < 6; ++l) {
                if (sg.left >= 0) a = a + Cn[36 * (size_t)sg.left + 6 * r + l] * Yg[78 * (size_t)first + 13 * l + c];
                if (sg.right >= 0) b = b + Cn[36 * (size_t)last + 6 * l + r] * Yg[78 * (size_t)last + 13 * l + c];
            }
            S[13 * r + c] = a;
            S[13 * (6 + r) + c] = b;
        }
    }
}

// Contribution codes of one lower block of the reduced system (ld = 6 |B|), in a fixed order:
//   (0 << 28) | v         D_v + lam I                    (diagonal blocks)
//   (1 << 28) | v         Cn_v^T   (block (v+1, v): chain factors between two separators)
//   (2 << 28) | f         H_ij^T of factor f, i < j      (3 << 28: H_ij, i > j)
//   (4 << 28) | 4 s + p   minus Schur part p of segment s: 0 LL, 1 RL (row R, column L), 3 RR
struct PgBlock {
    int32_t row, col;                  // separator positions, row >= col
    int32_t begin, end;                // contributions codes[begin, end)
};

__global__ void k_pg_reduced(const PgBlock *__restrict__ blocks, const int32_t *__restrict__ codes, int ld, double lam,
                             const double *__restrict__ D, const double *__restrict__ Cn, const double *__restrict__ H,
                             const double *__restrict__ schur, double *__restrict__ S)
{
    const PgBlock b = blocks[blockIdx.x];
    const int t = threadIdx.x;
    if (t >= 36) return;
    const int r = t / 6, c = t % 6;
    double s = 0.0;
    for (int p = b.begin; p < b.end; ++p) {
        const int code = codes[p], kind = code >> 28, id = code & 0x0fffffff;
        double x;
        if (kind == 0) x = D[36 * (size_t)id + t] + (r == c ? lam : 0.0);
        else if (kind == 1) x = Cn[36 * (size_t)id + 6 * c + r];
        else if (kind == 2) x = H[108 * (size_t)id + 72 + 6 * c + r];
        else if (kind == 3) x = H[108 * (size_t)id + 72 + 6 * r + c];
        else {
            const int sg = id >> 2, part = id & 3;
            const int rr = (part == 0) ? 0 : 6, cc = (part == 3) ? 6 : 0;   // rows L | R, columns L | R
            x = -schur[156 * (size_t)sg + 13 * (rr + r) + cc + c];
        }
        s = s + x;
    }
    S[(size_t)(6 * b.row + r) * ld + 6 * b.col + c] = s;
}

// right-hand side of separator a (compact node v): -g_v - Schur column 12 of its neighbouring segments
__global__ void k_pg_reduced_rhs(const int32_t *__restrict__ sep_node, const int32_t *__restrict__ sep_segs, int nb,
                                 const double *__restrict__ g, const double *__restrict__ schur, double *__restrict__ x)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 6 * nb) return;
    const int a = t / 6, r = t % 6;
    double s = -g[6 * (size_t)sep_node[a] + r];
    const int sl = sep_segs[2 * a], sr = sep_segs[2 * a + 1];   // segment ending at a (a is its right), starting at a
    if (sl >= 0) s = s - schur[156 * (size_t)sl + 13 * (6 + r) + 12];
    if (sr >= 0) s = s - schur[156 * (size_t)sr + 13 * r + 12];
    x[t] = s;
}

// ---- blocked right-looking Cholesky of the dense reduced matrix (lower, row-major, leading dimension ld = n)

__global__ __launch_bounds__(256) void k_chol_diag(double *__restrict__ S, int n, int k0, int *__restrict__ status)
{
    __shared__ double A[kCholNb][kCholNb + 1];
    const int nb = min(kCholNb, n - k0), t = threadIdx.x;
    for (int e = t; e < kCholNb * kCholNb; e += 256) {
        const int i = e / kCholNb, j = e % kCholNb;
        A[i][j] = (i < nb && j <= i) ? S[(size_t)(k0 + i) * n + k0 + j] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
        if (t == 0) {
            const double d = A[j][j];
            if (!(d > 0.0) || !isfinite(d)) *status = 1;
            A[j][j] = sqrt(d);
        }
        __syncthreads();
        for (int i = j + 1 + t; i < nb; i += 256) A[i][j] = A[i][j] / A[j][j];
        __syncthreads();
        for (int e = t; e < nb * nb; e += 256) {
            const int i = e / nb, c = e % nb;
            if (c > j && i >= c) A[i][c] = A[i][c] - A[i][j] * A[c][j];
        }
        __syncthreads();
    }
    for (int e = t; e < nb * nb; e += 256) {
        const int i = e / nb, j = e % nb;
        if (j <= i) S[(size_t)(k0 + i) * n + k0 + j] = A[i][j];
    }
}

// rows below the panel: X L^T = A, one row per thread
__global__ __launch_bounds__(64) void k_chol_panel(double *__restrict__ S, int n, int k0)
{
    __shared__ double L[kCholNb][kCholNb + 1];
    const int nb = min(kCholNb, n - k0), t = threadIdx.x;
    for (int e = t; e < kCholNb * kCholNb; e += 64) {
        const int i = e / kCholNb, j = e % kCholNb;
        L[i][j] = (i < nb && j <= i) ? S[(size_t)(k0 + i) * n + k0 + j] : 0.0;
    }
    __syncthreads();
    const int row = k0 + nb + blockIdx.x * 64 + t;
    if (row >= n) return;
    double x[kCholNb];
    double *a = S + (size_t)row * n + k0;
    for (int j = 0; j < kCholNb; ++j) {
        if (j >= nb) break;
        double s = a[j];
        for (int l = 0; l < j; ++l) s = s - x[l] * L[j][l];
        x[j] = s / L[j][j];
        a[j] = x[j];
    }
}

// trailing update of the lower triangle: A_ic -= sum_l P_il P_cl over the panel's columns, 32 x 32 tiles
__global__ __launch_bounds__(256) void k_chol_update(double *__restrict__ S, int n, int k0)
{
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi) return;
    __shared__ double Pi[kCholNb][kCholNb + 1], Pj[kCholNb][kCholNb + 1];
    const int nb = min(kCholNb, n - k0), base = k0 + nb, t = threadIdx.x;
    for (int e = t; e < kCholNb * kCholNb; e += 256) {
        const int r = e / kCholNb, l = e % kCholNb;
        const int ri = base + 32 * bi + r, rj = base + 32 * bj + r;
        Pi[r][l] = (ri < n && l < nb) ? S[(size_t)ri * n + k0 + l] : 0.0;
        Pj[r][l] = (rj < n && l < nb) ? S[(size_t)rj * n + k0 + l] : 0.0;
    }
    __syncthreads();
    for (int e = t; e < 32 * 32; e += 256) {
        const int r = e / 32, c = e % 32;
        const int i = base + 32 * bi + r, j = base + 32 * bj + c;
        if (i >= n || j > i) continue;
        double s = 0.0;
        for (int l = 0; l < nb; ++l) s = s + Pi[r][l] * Pj[c][l];
        S[(size_t)i * n + j] = S[(size_t)i * n + j] - s;
    }
}

// L y = b then L^T x = y in place, one workgroup; 32-row blocks solved by one wave with shuffles
__global__ __launch_bounds__(256) void k_trsv_pair(const double *__restrict__ S, int n, double *__restrict__ x)
{
    __shared__ double xb[32];
    __shared__ double Ld[32][33];
    const int t = threadIdx.x, lane = t & 63;
    const int nblk = (n + 31) / 32;
    for (int kb = 0; kb < nblk; ++kb) {
        const int r0 = 32 * kb, m = min(32, n - r0);
        for (int e = t; e < 32 * 32; e += 256) {      // the diagonal block into LDS: no dependent global loads below
            const int i = e / 32, j = e % 32;
            Ld[i][j] = (i < m && j <= i) ? S[(size_t)(r0 + i) * n + r0 + j] : 0.0;
        }
        __syncthreads();
        if (t < 64) {
            double val = (lane < m) ? x[r0 + lane] : 0.0;
            for (int j = 0; j < m; ++j) {
                if (lane == j) val = val / Ld[j][j];
                const double xj = __shfl(val, j);
                if (lane > j && lane < m) val = val - Ld[lane][j] * xj;
            }
            if (lane < m) {
                x[r0 + lane] = val;
                xb[lane] = val;
            }
        }
        __syncthreads();
        for (int i = r0 + m + t; i < n; i += 256) {
            double s = 0.0;
            for (int l = 0; l < m; ++l) s = s + S[(size_t)i * n + r0 + l] * xb[l];
            x[i] = x[i] - s;
        }
        __syncthreads();
    }
    for (int kb = nblk - 1; kb >= 0; --kb) {
        const int r0 = 32 * kb, m = min(32, n - r0);
        for (int e = t; e < 32 * 32; e += 256) {
            const int i = e / 32, j = e % 32;
            Ld[i][j] = (i < m && j <= i) ? S[(size_t)(r0 + i) * n + r0 + j] : 0.0;
        }
        __syncthreads();
        if (t < 64) {
            double val = (lane < m) ? x[r0 + lane] : 0.0;
            for (int j = m - 1; j >= 0; --j) {
                if (lane == j) val = val / Ld[j][j];
                const double xj = __shfl(val, j);
                if (lane < j) val = val - Ld[j][lane] * xj;
            }
            if (lane < m) {
                x[r0 + lane] = val;
                xb[lane] = val;
            }
        }
        __syncthreads();
        for (int i = t; i < r0; i += 256) {
            double s = 0.0;
            for (int l = 0; l < m; ++l) s = s + S[(size_t)(r0 + l) * n + i] * xb[l];
            x[i] = x[i] - s;
        }
        __syncthreads();
    }
}

// delta per node: node_seg[v] = segment of v, or -1 - (separator position) for a separator
__global__ void k_pg_backsub(const int32_t *__restrict__ node_seg, const PgSeg *__restrict__ segs,
                             const int32_t *__restrict__ sep_pos, const double *__restrict__ Yg,
                             const double *__restrict__ xb, int n, double *__restrict__ delta)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 6 * n) return;
    const int v = t / 6, r = t % 6, s = node_seg[v];
    if (s < 0) {
        delta[t] = xb[6 * (-1 - s) + r];
        return;
    }
    const PgSeg sg = segs[s];
    const double *Y = Yg + 78 * (size_t)v + 13 * r;
    double a = Y[12], u = 0.0;
    if (sg.left >= 0)
        for (int l = 0; l < 6; ++l) u = u + Y[l] * xb[6 * sep_pos[sg.left] + l];
    if (sg.right >= 0)
        for (int l = 0; l < 6; ++l) u = u + Y[6 + l] * xb[6 * sep_pos[sg.right] + l];
    delta[t] = a - u;
}

__global__ void k_pg_retract(const double *__restrict__ X, const double *__restrict__ delta, int n,
                             double *__restrict__ Xc)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    double E[12], out[12];
    se3_exp(delta + 6 * (size_t)v, E);
    se3_mul(X + 12 * (size_t)v, E, out);
    for (int e = 0; e < 12; ++e) Xc[12 * (size_t)v + e] = out[e];
}

// per factor: error at the candidate values, and the linearised error 0.5 ||A_i d_i + A_j d_j + rw||^2
__global__ void k_pg_trial(const PgFactor *__restrict__ fac, const int32_t *__restrict__ map, int F,
                           const double *__restrict__ Xc, const PgLin lin, const double *__restrict__ delta,
                           double *__restrict__ err_c, double *__restrict__ err_lin)
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
    err_c[f] = 0.5 * e;
    err_lin[f] = 0.5 * el;
}

// out[0] = sum a, out[1] = sum b (b may be null), fixed order: thread t sums t, t + 1024, ... then a fixed tree
__global__ __launch_bounds__(1024) void k_pg_reduce(const double *__restrict__ a, const double *__restrict__ b, int F,
                                                    double *__restrict__ out)
{
    __shared__ double sa[1024], sb[1024];
    const int t = threadIdx.x;
    double x = 0.0, y = 0.0;
    for (int f = t; f < F; f += 1024) {
        x = x + a[f];
        if (b) y = y + b[f];
    }
    sa[t] = x;
    sb[t] = y;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (t < w) {
            sa[t] = sa[t] + sa[t + w];
            sb[t] = sb[t] + sb[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[0] = sa[0];
        out[1] = sb[0];
    }
}

} // namespace icpmi
