// pose_graph_marginals.h -- selected blocks of H^-1 at the optimised poses: the joint marginal covariance
// of q queried poses, out of the structured factorisation pose_graph.h already produces (k_pg_segment, k_pg_reduced,
// k_chol_* at lam = 0).  With H = [A C; C^T B], A = diag(A_s) block tridiagonal per segment and S = B - C^T A^-1 C = L L^T,
// the columns of H^-1 that belong to node v are
//     x_B = S^-1 (e_B - C^T A^-1 e_A),    x_A = A^-1 e_A - (A^-1 C) x_B
// with (e_A, e_B) the six unit columns of v.  A^-1 C is k_pg_segment's Yg, columns 0-11.
//
//   k_pg_marg_segment    one workgroup per queried interior node: W = A_s^-1 E_v along its segment, and the two 6 x 6
//                        blocks -C^T W that reach the reduced system
//   k_pg_marg_rhs        the reduced right-hand sides, one 6|B| x 6 panel per queried node
//   k_pg_trsm_pair       L Y = R, L^T X = Y in place: k_trsv_pair's block scheme, one workgroup per panel
//   k_pg_marg_gather     block (a, b) of the answer
//
// fp64, every sum in a fixed order, no atomics.  A column's arithmetic is the same whichever panel or position it has
// and whatever else is queried, so a block of the answer does not depend on the query around it, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "pose_graph.h"

namespace icpmi {

constexpr int kPgTrsmThreads = 256;

// qnode[a]: compact node of the a-th queried pose.  W + a * wstride (wstride = 36 x the longest segment): W_k (6 x 6 row-major) for k along the segment;
// blk + 72 a: -Cn_L W_0 (rows of the left separator) then -Cn_last^T W_last (rows of the right one), zero where the
// separator does not exist.  Thread c < 6 owns column c from the first node to the last and back: a column of the
// recursion reads only itself.
__global__ __launch_bounds__(64) void k_pg_marg_segment(const int32_t *__restrict__ qnode,
                                                        const int32_t *__restrict__ node_seg,
                                                        const PgSeg *__restrict__ segs, const double *__restrict__ Cn,
                                                        const double *__restrict__ Lg, const double *__restrict__ Ug,
                                                        int wstride, double *__restrict__ W,
                                                        double *__restrict__ blk)
{
    const int a = blockIdx.x, t = threadIdx.x;
    const int v = qnode[a], s = node_seg[v];
    if (s < 0) return;                                   // a separator: its columns start in the reduced system
    const PgSeg sg = segs[s];
    const int p = v - sg.start;
    double *Wa = W + (size_t)wstride * a;
    if (t < 6) {
        const int c = t;
        double x[6] = {0, 0, 0, 0, 0, 0};                // V_{k-1}, zero before p
        for (int k = 0; k < sg.len; ++k) {
            const double *L = Lg + 36 * (size_t)(sg.start + k);
            if (k >= p) {
                double w[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    double e = (k == p && i == c) ? 1.0 : 0.0;
                    if (k > p) {
                        const double *Up = Ug + 36 * (size_t)(sg.start + k - 1);
                        double u = 0.0;
#pragma unroll
                        for (int l = 0; l < 6; ++l) u = u + Up[6 * l + i] * x[l];
                        e = e - u;
                    }
                    w[i] = e;
                }
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    double e = w[i];
#pragma unroll
                    for (int l = 0; l < 6; ++l)
                        if (l < i) e = e - L[6 * i + l] * x[l];
                    x[i] = e / L[6 * i + i];
                }
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) Wa[36 * k + 6 * i + c] = x[i];
        }
        double y[6] = {0, 0, 0, 0, 0, 0};
        for (int k = sg.len - 1; k >= 0; --k) {
            const double *L = Lg + 36 * (size_t)(sg.start + k), *U = Ug + 36 * (size_t)(sg.start + k);
            double w[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double e = Wa[36 * k + 6 * i + c];
                if (k < sg.len - 1) {
                    double u = 0.0;
#pragma unroll
                    for (int l = 0; l < 6; ++l) u = u + U[6 * i + l] * y[l];
                    e = e - u;
                }
                w[i] = e;
            }
#pragma unroll
            for (int i = 5; i >= 0; --i) {
                double e = w[i];
#pragma unroll
                for (int l = 5; l >= 0; --l)
                    if (l > i) e = e - L[6 * l + i] * y[l];
                y[i] = e / L[6 * i + i];
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) Wa[36 * k + 6 * i + c] = y[i];
        }
    }
    __syncthreads();
    if (t < 36) {
        const int r = t / 6, c = t % 6;
        double left = 0.0, right = 0.0;
        const double *W0 = Wa, *Wl = Wa + 36 * (size_t)(sg.len - 1);
        if (sg.left >= 0) {
            const double *C = Cn + 36 * (size_t)sg.left;
            for (int l = 0; l < 6; ++l) left = left + C[6 * r + l] * W0[6 * l + c];
            left = -left;
        }
        if (sg.right >= 0) {
            const double *C = Cn + 36 * (size_t)(sg.start + sg.len - 1);
            for (int l = 0; l < 6; ++l) right = right + C[6 * l + r] * Wl[6 * l + c];
            right = -right;
        }
        blk[72 * (size_t)a + t] = left;
        blk[72 * (size_t)a + 36 + t] = right;
    }
}

// X + a * (6 nr): the panel of queried node a, nr rows of 6 columns.  Every entry has one owner.
__global__ void k_pg_marg_rhs(const int32_t *__restrict__ qnode, const int32_t *__restrict__ node_seg,
                              const PgSeg *__restrict__ segs, const int32_t *__restrict__ sep_pos,
                              const double *__restrict__ blk, int q, int nr, double *__restrict__ X)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)q * nr * 6) return;
    const int a = (int)(e / ((size_t)nr * 6)), rem = (int)(e % ((size_t)nr * 6));
    const int row = rem / 6, c = rem % 6, sp = row / 6, r = row % 6;
    const int v = qnode[a], s = node_seg[v];
    double x = 0.0;
    if (s < 0) {
        if (-1 - s == sp && r == c) x = 1.0;
    } else {
        const PgSeg sg = segs[s];
        if (sg.left >= 0 && sep_pos[sg.left] == sp) x = blk[72 * (size_t)a + 6 * r + c];
        else if (sg.right >= 0 && sep_pos[sg.right] == sp) x = blk[72 * (size_t)a + 36 + 6 * r + c];
    }
    X[e] = x;
}

// L Y = R then L^T X = Y in place for the six columns of one panel per workgroup (S: the reduced Cholesky factor, lower,
// row-major, leading dimension n).  Per 32-row diagonal block: wave 0 solves the block out of LDS, lane = row, the six
// columns side by side in registers; then all threads update the rows below (backward: above), each loading its piece
// of L once for the six columns.
__global__ __launch_bounds__(kPgTrsmThreads) void k_pg_trsm_pair(const double *__restrict__ S, int n,
                                                                 double *__restrict__ Xall)
{
    __shared__ double xb[32][6];
    __shared__ double Ld[32][33];
    double *X = Xall + (size_t)blockIdx.x * n * 6;
    const int t = threadIdx.x, lane = t & 63;
    const int nblk = (n + 31) / 32;
    for (int kb = 0; kb < nblk; ++kb) {
        const int r0 = 32 * kb, m = min(32, n - r0);
        for (int e = t; e < 32 * 32; e += kPgTrsmThreads) {
            const int i = e / 32, j = e % 32;
            Ld[i][j] = (i < m && j <= i) ? S[(size_t)(r0 + i) * n + r0 + j] : 0.0;
        }
        __syncthreads();
        if (t < 64) {
            const bool live = lane < m;
            double val[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) val[c] = live ? X[(size_t)(r0 + lane) * 6 + c] : 0.0;
            const double dinv = live ? 1.0 / Ld[lane & 31][lane & 31] : 0.0;   // one division per row, not per step
            for (int j = 0; j < m; ++j) {
                const double lj = live ? Ld[lane & 31][j] : 0.0;
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    const double q = val[c] * dinv;
                    val[c] = (lane == j) ? q : val[c];
                    const double xj = __shfl(val[c], j);
                    const double u = val[c] - lj * xj;
                    val[c] = (lane > j && live) ? u : val[c];
                }
            }
            if (live) {
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    X[(size_t)(r0 + lane) * 6 + c] = val[c];
                    xb[lane][c] = val[c];
                }
            }
        }
        __syncthreads();
        for (int i = r0 + m + t; i < n; i += kPgTrsmThreads) {
            const double *Li = S + (size_t)i * n + r0;
            double s[6] = {0, 0, 0, 0, 0, 0};
            for (int l = 0; l < m; ++l) {
                const double a = Li[l];
#pragma unroll
                for (int c = 0; c < 6; ++c) s[c] = s[c] + a * xb[l][c];
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) X[(size_t)i * 6 + c] = X[(size_t)i * 6 + c] - s[c];
        }
        __syncthreads();
    }
    for (int kb = nblk - 1; kb >= 0; --kb) {
        const int r0 = 32 * kb, m = min(32, n - r0);
        for (int e = t; e < 32 * 32; e += kPgTrsmThreads) {
            const int i = e / 32, j = e % 32;
            Ld[i][j] = (i < m && j <= i) ? S[(size_t)(r0 + i) * n + r0 + j] : 0.0;
        }
        __syncthreads();
        if (t < 64) {
            const bool live = lane < m;
            double val[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) val[c] = live ? X[(size_t)(r0 + lane) * 6 + c] : 0.0;
            const double dinv = live ? 1.0 / Ld[lane & 31][lane & 31] : 0.0;
            for (int j = m - 1; j >= 0; --j) {
                const double lj = live ? Ld[j][lane & 31] : 0.0;   // zero above the diagonal
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    const double q = val[c] * dinv;
                    val[c] = (lane == j) ? q : val[c];
                    const double xj = __shfl(val[c], j);
                    const double u = val[c] - lj * xj;
                    val[c] = (lane < j) ? u : val[c];
                }
            }
            if (live) {
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    X[(size_t)(r0 + lane) * 6 + c] = val[c];
                    xb[lane][c] = val[c];
                }
            }
        }
        __syncthreads();
        for (int i = t; i < r0; i += kPgTrsmThreads) {
            double s[6] = {0, 0, 0, 0, 0, 0};
            for (int l = 0; l < m; ++l) {
                const double a = S[(size_t)(r0 + l) * n + i];
#pragma unroll
                for (int c = 0; c < 6; ++c) s[c] = s[c] + a * xb[l][c];
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) X[(size_t)i * 6 + c] = X[(size_t)i * 6 + c] - s[c];
        }
        __syncthreads();
    }
}

// out (6q x 6q row-major): block (a, b) = rows of node u = qnode[a], columns of node v = qnode[b].  A separator's rows
// come from the reduced solve; an interior node's by k_pg_backsub's rule, with W_v[u] where v lies in u's segment.
__global__ __launch_bounds__(64) void k_pg_marg_gather(const int32_t *__restrict__ qnode,
                                                       const int32_t *__restrict__ node_seg,
                                                       const PgSeg *__restrict__ segs, const int32_t *__restrict__ sep_pos,
                                                       const double *__restrict__ Yg, const double *__restrict__ W,
                                                       int wstride, const double *__restrict__ X, int q, int nr,
                                                       double *__restrict__ out)
{
    const int a = blockIdx.x / q, b = blockIdx.x % q, t = threadIdx.x;
    if (t >= 36) return;
    const int r = t / 6, c = t % 6;
    const int u = qnode[a], v = qnode[b], su = node_seg[u];
    const double *Xb = X + (size_t)b * nr * 6;
    double res;
    if (su < 0) {
        res = Xb[(size_t)(6 * (-1 - su) + r) * 6 + c];
    } else {
        const PgSeg sg = segs[su];
        const double *Y = Yg + 78 * (size_t)u + 13 * r;
        const double w = (node_seg[v] == su) ? W[(size_t)wstride * b + 36 * (size_t)(u - sg.start) + 6 * r + c] : 0.0;
        double acc = 0.0;
        if (sg.left >= 0)
            for (int l = 0; l < 6; ++l) acc = acc + Y[l] * Xb[(size_t)(6 * sep_pos[sg.left] + l) * 6 + c];
        if (sg.right >= 0)
            for (int l = 0; l < 6; ++l) acc = acc + Y[6 + l] * Xb[(size_t)(6 * sep_pos[sg.right] + l) * 6 + c];
        res = w - acc;
    }
    out[(size_t)(6 * a + r) * (6 * (size_t)q) + 6 * b + c] = res;
}

} // namespace icpmi
