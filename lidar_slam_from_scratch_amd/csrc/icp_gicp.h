// icp_gicp.h -- plane-to-plane (generalized) ICP (icpmi_align_gicp*).
//
// Both clouds carry a local surface model: the plane-regularised covariance U diag(1, 1, epsilon) U^T of a row with unit
// normal n is I - (1 - epsilon) n n^T, so the normals are all either side needs and no eigendecomposition is run.
//
// Per pass, for row i of the moved source `cur` with nearest target j (`found` as in k_reduce_rule), in unfused fp64 and in
// this order:
//     R    = rotation block of IcpState::total as the pass finds it (total[0..2], [4..6], [8..10])
//     s    = normal of source row i, estimated ONCE per call on the source as the caller gave it
//            (before initial_transform; k = options.normal_k; the normals launch_normals gives)
//     m_a  = (R[a][0]*s0 + R[a][1]*s1) + R[a][2]*s2
//     n    = normal of target j;  p = cur_i;  e = q_j - p;  d2 = (e0*e0 + e1*e1) + e2*e2
//     kept iff found && d2 <= g2      (g2 = max_distance^2, or DBL_MAX when max_distance == 0)
//     c = 1 - epsilon, kappa = 2*epsilon            (formed once on the host)
//     S_ab = (a==b ? 2.0 : 0.0) - c*(n_a*n_b + m_a*m_b)          for a <= b
//     C00 = S11*S22 - S12*S12;  C01 = S02*S12 - S01*S22;  C02 = S01*S12 - S02*S11
//     C11 = S00*S22 - S02*S02;  C12 = S01*S02 - S00*S12;  C22 = S00*S11 - S01*S01
//     det = (S00*C00 + S01*C01) + S02*C02;  r = 1.0/det;  M_ab = C_ab*r      (one division per kept row)
//     u_a = (M_a0*e0 + M_a1*e1) + M_a2*e2
//     A   = [ -[p]x | I ]:  A0 = (0, p2, -p1, 1,0,0), A1 = (-p2, 0, p0, 0,1,0), A2 = (p1, -p0, 0, 0,0,1)
//     B   = [p]x M (rows 0..2 against columns 3..5 of A^T M A; M_ab = M_ba):
//           B0c = p1*M2c - p2*M1c;  B1c = p2*M0c - p0*M2c;  B2c = p0*M1c - p1*M0c
//     G   = B (-[p]x) (rows and columns 0..2), for r <= c only:
//           Gr0 = Br2*p1 - Br1*p2;  Gr1 = Br0*p2 - Br2*p0;  Gr2 = Br1*p0 - Br0*p1
//     v   = p x u:  v0 = p1*u2 - p2*u1;  v1 = p2*u0 - p0*u2;  v2 = p0*u1 - p1*u0
// Columns of a kept row (k_reduce_gated's layout; a dropped row adds nothing):
//     0..20   the upper triangle of A^T M A, row by row:
//             G00 G01 G02 B00 B01 B02 | G11 G12 B10 B11 B12 | G22 B20 B21 B22 | M00 M01 M02 | M11 M12 | M22
//     21..26  A^T u = v0 v1 v2 u0 u1 u2
//     27      kappa * ((e0*u0 + e1*u1) + e2*u2)
//     28      1.0
// The step solves H x = g with H = sum A^T M A, g = sum A^T M e; in the point-to-plane limit M = n n^T these are J J^T and
// J b, so k_finish_step_gated and k_transform run unchanged.
// error = sqrt(sums[27] / sums[28]).  kappa makes it read in metres: with parallel normals M = diag(1/(2 epsilon), 1/2, 1/2)
// in the normal's frame, so kappa e^T M e = (e.n)^2 + epsilon * (tangential)^2 -- the point-to-plane RMS plus a small
// tangential term -- and the reference node's `> 1.0`, a loop detector's `< 0.3` and `tolerance` keep their meaning.
// epsilon = 1 gives S = 2 I and M = I / 2 exactly: point-to-point ICP.
// The no-pairs rule, the step, the composition, the post-loop entry and the history invariants are icp_gated.h's.
// A non-finite source row is dropped by the d2 test (its normal is whatever the source's k-NN pass gave it).
//
//   k_reduce_gicp         k_reduce_gated's grid, block, grid-stride loop, wave / LDS reduction and partial-row store around
//                         a body of its own (icp_gicp_row.inc, included as text: the arithmetic sits in the kernel)
//   k_finish_step_gated   reused as it is (icp_gated.h);  k_transform likewise.
//   k_icp_small_gicp      icp_small_kernel.inc's fourth expansion (ICPMI_SMALL_GATED 1, ICPMI_SMALL_GICP 1): the gated
//                         small-cloud kernel with step 4's row formed by the same text from the winner it holds.  R is loaded
//                         with the state at the top of the kernel and m formed per row beside step 1's move; a dropped row
//                         leaves 28 zeros and count 0.  Its rows are added in the small-cloud kernel's order (a wave's four
//                         rows, the waves, then k_finish_step_gated's), not k_reduce_gicp's: the two forms agree to rounding,
//                         not to bits, so the form is the caller's choice (ICPMI_GICP_FORM_SMALL) and off by default.
#pragma once
#include "icp_gated.h"
#include "kernels.h"

namespace icpmi {

// (the partial row is the gate's: 28 sums and the kept rows)
static_assert(RuleGate::kCols == 29 && kNumSums == 29, "k_finish_step_gated sums the columns k_reduce_gicp leaves");

__global__ __launch_bounds__(256) void k_reduce_gicp(const double *__restrict__ cur, int n, const double *__restrict__ tgt, int m_tgt,
                                                     const double *__restrict__ nrm, const int *__restrict__ idx,
                                                     const double *__restrict__ src_nrm, double *__restrict__ partials,
                                                     const IcpState *__restrict__ st, const double g2, const double c,
                                                     const double kappa)
{
    if (st->done) return;
    // wave-uniform: nine scalar loads per thread, not per row
    const double R00 = st->total[0], R01 = st->total[1], R02 = st->total[2];
    const double R10 = st->total[4], R11 = st->total[5], R12 = st->total[6];
    const double R20 = st->total[8], R21 = st->total[9], R22 = st->total[10];
    double acc[29]; // (acc[28]: the kept rows, a small integer, exact in any order of additions)
#pragma unroll
    for (int k = 0; k < 29; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int ji = idx[i];
        const bool found = (unsigned)ji < (unsigned)m_tgt; // (-1: a non-finite row has no neighbour, kdtree.hpp:53)
        const int j = found ? ji : 0;                      // the gather stays in bounds
        const double p0 = cur[3 * i], p1 = cur[3 * i + 1], p2 = cur[3 * i + 2];
        const double q0 = tgt[3 * j], q1 = tgt[3 * j + 1], q2 = tgt[3 * j + 2];
        const double n0 = nrm[3 * j], n1 = nrm[3 * j + 1], n2 = nrm[3 * j + 2];
        const double s0 = src_nrm[3 * i], s1 = src_nrm[3 * i + 1], s2 = src_nrm[3 * i + 2];
        const double e0 = q0 - p0, e1 = q1 - p1, e2 = q2 - p2;
        if (!(found && (e0 * e0 + e1 * e1) + e2 * e2 <= g2)) continue; // dropped: nothing is added, not even a zero
#define ICPMI_GICP_PART 1
#include "icp_gicp_row.inc"
#undef ICPMI_GICP_PART
#define ICPMI_GICP_PART 2
#define ICPMI_GICP_COL(k, value) acc[k] += (value);
#include "icp_gicp_row.inc"
#undef ICPMI_GICP_COL
#undef ICPMI_GICP_PART
    }
    __shared__ double red[4][29];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 29; ++k) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 29) {
        const int k = threadIdx.x;
        partials[(size_t)blockIdx.x * kSumsStride + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

#define ICPMI_SMALL_ROBUST 0
#define ICPMI_SMALL_GATED 1
#define ICPMI_SMALL_GICP 1
#include "icp_small_kernel.inc"
#undef ICPMI_SMALL_GICP
#undef ICPMI_SMALL_GATED
#undef ICPMI_SMALL_ROBUST

} // namespace icpmi
