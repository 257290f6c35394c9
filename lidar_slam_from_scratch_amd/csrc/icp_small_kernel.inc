// icp_small_kernel.inc -- the text of the small-cloud kernel (icp_small.h), included twice: with ICPMI_SMALL_GATED 0 it is
// k_icp_small, token for token what it was before the correspondence-distance gate existed (so its instructions are too),
// with ICPMI_SMALL_GATED 1 it is k_icp_small_gated (icp_gated.h): the same kernel with the gate's test on the winner that
// step 4 already holds, and the kept count in column 28 of the partial row.  With ICPMI_SMALL_ROBUST 1 as well (icp_robust.h)
// it is k_icp_small_robust: the gated kernel with the row's weight on its terms, the weight in column 28 and the kept
// count in column 29.  With ICPMI_SMALL_GATED 1 and ICPMI_SMALL_GICP 1 (icp_gicp.h) it is k_icp_small_gicp: the gated
// kernel with step 4's row formed by icp_gicp_row.inc from the winner it holds and the row's source normal.  The other
// expansions stay token for token what they were.
#if ICPMI_SMALL_GICP
#define ICPMI_SMALL_COLS 29 // the gate's partial row: the 28 plane-to-plane sums and the kept count
__global__ __launch_bounds__(kSmallThreads) void k_icp_small_gicp(
#elif ICPMI_SMALL_ROBUST
#define ICPMI_SMALL_COLS 30 // the 28 weighted sums, the weight sum and the kept count
__global__ __launch_bounds__(kSmallThreads) void k_icp_small_robust(
#elif ICPMI_SMALL_GATED
#define ICPMI_SMALL_COLS 29 // columns of a partial row the kernel forms: the 28 sums and the kept count
__global__ __launch_bounds__(kSmallThreads) void k_icp_small_gated(
#else
#define ICPMI_SMALL_COLS 28
__global__ __launch_bounds__(kSmallThreads) void k_icp_small(
#endif
    const double *in, double *cur, int n, const IcpState *__restrict__ st, int which,
    const uint4 *__restrict__ Bpack, const SplitFrame *__restrict__ frames, int splits,
    const double *__restrict__ sorted, const double *__restrict__ nrm_sorted, const unsigned *__restrict__ perm,
    int m, int ms, const double *__restrict__ tgt_orig, const double *__restrict__ nrm,
    double *__restrict__ partials, unsigned long long *__restrict__ counters
#if ICPMI_SMALL_GATED
    , const double g2 // max_distance^2, formed once on the host (icp_gated.h)
#endif
#if ICPMI_SMALL_ROBUST
    , const int kind, const double ks // the weight and its scale (icp_robust.h: k for Huber, k * k for Geman-McClure)
#endif
#if ICPMI_SMALL_GICP
    , const double *__restrict__ src_nrm, const double c, const double kappa // the source's normals in the caller's row order, 1 - epsilon, 2 * epsilon (icp_gicp.h)
#endif
    )
{
    __shared__ uint4 scratch[kSmallWaves][32 * 36 / 4]; // per wave: A rows, then the epilogue's transpose
    __shared__ float2 rec[kSmallMaxSplits * kSmallUnitsPerSplit][kSmallQ];
#if ICPMI_SMALL_ROBUST
    __shared__ double jrow[kSmallQ][31]; // (an odd stride, as 29 is)
#else
    __shared__ double jrow[kSmallQ][29];
#endif
    __shared__ double red[kSmallWaves][ICPMI_SMALL_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = blockIdx.x * kSmallQ;
    const int nunits = splits * kSmallUnitsPerSplit;

    // Everything the kernel needs first is requested at once, oldest first what is needed first (vector loads
    // return in order): the state (is the loop over? the pending pose update), the rows, then the B operands
    // of the wave's first unit -- ONE trip to memory, the loop-ended test behind the requests.
    const int done = st->done;
    const double *T = which ? st->total : st->delta;
    const double r00 = T[0], r01 = T[1], r02 = T[2], t0 = T[3];
    const double r10 = T[4], r11 = T[5], r12 = T[6], t1 = T[7];
    const double r20 = T[8], r21 = T[9], r22 = T[10], t2 = T[11];
    const int iq = q0 + (lane & 31) < n ? q0 + (lane & 31) : n - 1;
    double x = in[3 * iq], y = in[3 * iq + 1], z = in[3 * iq + 2];
    asm volatile("" : "+v"(x), "+v"(y), "+v"(z)); // (the row loads stay in front of the operand loads and of the test below)
#if ICPMI_SMALL_GICP
    // the rotation of IcpState::total as the pass finds it -- the pose the rows have once step 1 has moved them, in the first
    // pass (T is total itself) and in the later ones (k_finish_step_gated has composed the step into it) -- and the row's
    // source normal, with the state and the rows: wave-uniform words and one more row load of the same trip
    const double R00 = st->total[0], R01 = st->total[1], R02 = st->total[2];
    const double R10 = st->total[4], R11 = st->total[5], R12 = st->total[6];
    const double R20 = st->total[8], R21 = st->total[9], R22 = st->total[10];
    const double s0 = src_nrm[3 * iq], s1 = src_nrm[3 * iq + 1], s2 = src_nrm[3 * iq + 2];
#endif
    int u = wave;
    uint4 b[kSmallUnitTiles];
    if (u < nunits) {
        const uint4 *tiles = Bpack + (size_t)u * (kSmallUnitTiles * 64) + lane; // unit u = tiles [32 u, 32 u + 32) of the packed array
#pragma unroll
        for (int tt = 0; tt < kSmallUnitTiles; ++tt) b[tt] = tiles[tt * 64];
    }
    if (done) return; // the loop has ended: the source stays where it is (icp.hpp:210-217)
    // 1. the workgroup's 32 rows, lanes l and l + 32 of every wave holding row l & 31, moved by the pending
    // update (icp.hpp:174-176 / :225-226, k_transform's operation order)
    const double px = ((x * r00 + y * r01) + z * r02) + t0;
    const double py = ((x * r10 + y * r11) + z * r12) + t1;
    const double pz = ((x * r20 + y * r21) + z * r22) + t2;
#if ICPMI_SMALL_GICP
    // (the source normal in the target frame, per row like px: three words live through the coarse pass, R and s are dead)
#define ICPMI_GICP_PART 1
#include "icp_gicp_row.inc"
#undef ICPMI_GICP_PART
#endif

    // 2. coarse records of this wave's units
    f32x16 zero;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero[r] = 0.f;
#pragma unroll 1
    while (u < nunits) {
        const int s = u / kSmallUnitsPerSplit;
        bf16x8 afrag;
        float pn;
        {
            const float fx = (float)(px - frames[s].c[0]), fy = (float)(py - frames[s].c[1]), fz = (float)(pz - frames[s].c[2]);
            unsigned xh, xm, yh, ym, zh, zm;
            split2(fx, xh, xm);
            split2(fy, yh, ym);
            split2(fz, zh, zm);
            const float tx = __uint_as_float(xh << 16) + __uint_as_float(xm << 16);
            const float ty = __uint_as_float(yh << 16) + __uint_as_float(ym << 16);
            const float tz = __uint_as_float(zh << 16) + __uint_as_float(zm << 16);
            pn = (tx * tx + ty * ty) + tz * tz; // |P|^2 of the represented point (coarse_build_a)
            const unsigned pnh = __float_as_uint(pn) >> 16;
            pn -= __uint_as_float(pnh << 16);
            const unsigned one = 0x3f80u;
            // (lanes l and l + 32 formed the same row: the lower keeps its first half, the upper its second -- the MFMA's A
            // fragment, without the trip through LDS it took until round 4)
            const uint4 u0 = make_uint4(xh | (xh << 16), xm | (xm << 16), yh | (yh << 16), ym | (ym << 16));
            const uint4 u1 = make_uint4(zh | (zh << 16), zm | (zm << 16), one | (one << 16), one | (pnh << 16));
            afrag = __builtin_bit_cast(bf16x8, lane < 32 ? u0 : u1);
        }
        f32x16 mn;
#pragma unroll
        for (int r = 0; r < 16; ++r) mn[r] = kBig;
#pragma unroll
        for (int tt = 0; tt < kSmallUnitTiles; tt += 2) {
            const f32x16 da = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afrag, __builtin_bit_cast(bf16x8, b[tt]), zero, 0, 0, 0);
            const f32x16 db = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afrag, __builtin_bit_cast(bf16x8, b[tt + 1]), zero, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) mn[r] = min3f(mn[r], da[r], db[r]);
        }
        // epilogue (coarse_epilogue, MODE 0): transpose, tag, top two of the 32 columns, + the rest of |P|^2
        {
            float *sc = reinterpret_cast<float *>(scratch[wave]);
            const int ql = lane & 31, half = lane >> 5;
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[((r & 3) + 8 * (r >> 2) + 4 * half) * 36 + ql] = mn[r];
            __builtin_amdgcn_wave_barrier();
            float v[16];
            const float4 *rowp = reinterpret_cast<const float4 *>(sc + ql * 36 + half * 16);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float4 xx = rowp[e];
                v[4 * e] = xx.x, v[4 * e + 1] = xx.y, v[4 * e + 2] = xx.z, v[4 * e + 3] = xx.w;
            }
            __builtin_amdgcn_wave_barrier();
            float v1 = kBig, v2 = kBig;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const float xx = tag_low5(v[c], (unsigned)c);
                v2 = med3_raw(v1, v2, xx);
                v1 = min_raw(v1, xx);
            }
            const unsigned col = (__float_as_uint(v1) & 15u) | ((unsigned)half << 4);
            v1 = tag_low5(min_raw(__uint_as_float(__float_as_uint(v1) & 0xFFFFFFE0u) + pn, kBig), col);
            v2 = min_raw(__uint_as_float(__float_as_uint(v2) & 0xFFFFFFE0u) + pn, kBig);
            const float o1 = lane_xor<32>(v1), o2 = lane_xor<32>(v2);
            const float hi = __builtin_fmaxf(v1, o1);
            v1 = __builtin_fminf(v1, o1);
            v2 = min3f(hi, v2, o2);
            if (half == 0) rec[u][ql] = make_float2(v1, v2);
        }
        u += kSmallWaves;
        if (u < nunits) { // (targets of more than four splits: the next unit's operands)
            const uint4 *tiles = Bpack + (size_t)u * (kSmallUnitTiles * 64) + lane;
#pragma unroll
            for (int tt = 0; tt < kSmallUnitTiles; ++tt) b[tt] = tiles[tt * 64];
        }
    }
    __syncthreads(); // records complete; every wave has read the old rows of `in`
    if (wave == 0 && lane < 32 && q0 + lane < n) {
        cur[3 * (q0 + lane)] = px;
        cur[3 * (q0 + lane) + 1] = py;
        cur[3 * (q0 + lane) + 2] = pz;
    }

    // 3. resolve, one row per quarter-wave (k_nn_resolve4): lane ql of the quarter holds split ql's record.
    // (Measured and dropped: the steps in leaner layouts -- selection and terms one lane per row in wave 0, the
    // certificate one lane per (row, split) -- with the rows' state handed on through LDS: fewer instructions, but
    // three more workgroup barriers, each waiting for the wave whose operands arrived last: 23.3 us per
    // iteration against 20.3.)
    const int quarter = lane >> 4, ql = lane & 15;
    const int qi = wave * 4 + quarter;
    const bool valid = q0 + qi < n;
    const double qx = __shfl(px, qi, 64), qy = __shfl(py, qi, 64), qz = __shfl(pz, qi, 64);
#if ICPMI_SMALL_GICP
    const double qm0 = __shfl(m0, qi, 64), qm1 = __shfl(m1, qi, 64), qm2 = __shfl(m2, qi, 64);
#endif
    float v1 = kBig, v2 = kBig;
    if (ql < splits) {
        const float2 a = rec[ql * kSmallUnitsPerSplit][qi];
        v1 = a.x, v2 = a.y;
#pragma unroll
        for (int h = 1; h < kSmallUnitsPerSplit; ++h) {
            const float2 w = rec[ql * kSmallUnitsPerSplit + h][qi];
            small_merge(v1, v2, w.x, w.y);
        }
    }
    int bs = ql < splits ? ql : 0x7fffffff;
    int bcol;
    {
        float best = v1;
#define ICPMI_STEP(S)                                                                     \
        {                                                                                 \
            const float ov = row16_partner<S>(best);                                      \
            const int os = row16_partner<S>(bs);                                          \
            const bool take = (ov < best) | ((ov == best) & (os < bs));                   \
            best = take ? ov : best;                                                      \
            bs = take ? os : bs;                                                          \
        }
        ICPMI_STEP(0) ICPMI_STEP(1) ICPMI_STEP(2) ICPMI_STEP(3) // (device_math.h: DPP partners, no LDS trip)
#undef ICPMI_STEP
        bcol = (int)(__float_as_uint(best) & 31u);
    }

    // exact scan of the winning slot: lane ql takes sorted positions ql, ql + 16, ... of it, each candidate's
    // NORMAL fetched next to its coordinates; the lane that ends up holding the winner has the matched point
    // and its normal in registers
    double ld = 1.7976931348623157e308, lq0 = 0.0, lq1 = 0.0, lq2 = 0.0, ln0 = 0.0, ln1 = 0.0, ln2 = 0.0;
    int lj = 0x7fffffff;
    {
        const int j0 = bs * kSplitTargets + bcol * kSlotTargets + ql;
        double cx[4], cy[4], cz[4], a0[4], a1[4], a2[4];
        int oj[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int jj = j0 + 16 * o;
            const int jc = jj < m ? jj : m - 1;
            cx[o] = ICPMI_SX(sorted, ms, jc), cy[o] = ICPMI_SY(sorted, ms, jc), cz[o] = ICPMI_SZ(sorted, ms, jc);
            a0[o] = ICPMI_SX(nrm_sorted, ms, jc), a1[o] = ICPMI_SY(nrm_sorted, ms, jc), a2[o] = ICPMI_SZ(nrm_sorted, ms, jc);
            oj[o] = (int)perm[jc];
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int jj = j0 + 16 * o;
            const double dd = sqdist(cx[o], cy[o], cz[o], qx, qy, qz);
            if (jj < m && (dd < ld || (dd == ld && oj[o] < lj))) {
                ld = dd, lj = oj[o];
                lq0 = cx[o], lq1 = cy[o], lq2 = cz[o];
                ln0 = a0[o], ln1 = a1[o], ln2 = a2[o];
            }
        }
    }
    double bd = ld;
    int bj = lj;
    row16_argmin(bd, bj);

    // certificate: every split's record against its bound (resolve_certify without the first filter:
    // there are at most 16 splits, one per lane of the quarter)
    {
        const double sq = sqrt(bd);
        const bool look = valid && finite3(qx, qy, qz);
        bool whole = false, slot = false;
        if (ql < splits && look) {
            const float tauf = split_tau(qx, qy, qz, frames[ql], bd, sq);
            whole = v2 <= tauf;
            slot = !whole && ql != bs && v1 <= tauf;
        }
        unsigned long long pend = __ballot(whole || slot);
        while (pend) { // rare; wave-uniform loop
            const int L = __ffsll((long long)pend) - 1;
            pend &= pend - 1;
            const double sx = __shfl(qx, L, 64), sy = __shfl(qy, L, 64), sz = __shfl(qz, L, 64);
            const int w = __shfl((int)whole, L, 64);
            const int c = __shfl((int)(__float_as_uint(v1) & 31u), L, 64);
            const int sL = L & 15;
            double d = 1.7976931348623157e308;
            int j = 0x7fffffff;
            if (w)
                scan_split<2>(sorted, perm, m, ms, reinterpret_cast<const double *>(frames + splits), sL, sx, sy, sz,
                              __shfl(bd, L, 64), lane, d, j);
            else scan_range<kSlotTargets, 1>(sorted, perm, m, ms, sL * kSplitTargets + c * kSlotTargets, sx, sy, sz, lane, d, j);
            if ((lane >> 4) == (L >> 4) && (d < bd || (d == bd && j < bj))) {
                bd = d;
                bj = j;
            }
            if (counters && lane == L) atomicAdd(&counters[w ? 1 : 0], 1ull);
        }
    }

    // 4. J row and b (icp.hpp:99-117) by the lane that holds the winner's point and normal; if the certificate
    // moved the winner out of the scanned slot (a few rows in a thousand) or the row has no neighbour
    // (non-finite: index 0 stands in, as in the general path), lane 0 of the quarter gathers by original index
    {
        bool have = valid && lj == bj && bj != 0x7fffffff;
        const unsigned long long anyhave = __ballot(have) & (0xFFFFull << (16 * quarter));
        if (valid && !anyhave && ql == 0) {
            const int j = (unsigned)bj < (unsigned)m ? bj : 0;
            lq0 = tgt_orig[3 * j], lq1 = tgt_orig[3 * j + 1], lq2 = tgt_orig[3 * j + 2];
            ln0 = nrm[3 * j], ln1 = nrm[3 * j + 1], ln2 = nrm[3 * j + 2];
            have = true;
        }
        if (have) {
#if ICPMI_SMALL_GICP
            // the gate's test as below, then the kept row's 29 columns by icp_gicp_row.inc, the text k_reduce_gicp includes: a
            // dropped row leaves 28 zeros and count 0, a kept row count 1 (column 28)
            const double e0 = lq0 - qx, e1 = lq1 - qy, e2 = lq2 - qz;
            double *row = jrow[qi];
            const bool keep = (e0 * e0 + e1 * e1) + e2 * e2 <= g2;
            if (!keep) {
#pragma unroll
                for (int e = 0; e < 29; ++e) row[e] = 0.0;
            } else {
                const double p0 = qx, p1 = qy, p2 = qz, n0 = ln0, n1 = ln1, n2 = ln2, m0 = qm0, m1 = qm1, m2 = qm2;
#define ICPMI_GICP_PART 2
#define ICPMI_GICP_COL(k, value) row[k] = (value);
#include "icp_gicp_row.inc"
#undef ICPMI_GICP_COL
#undef ICPMI_GICP_PART
            }
#else
            double J[6];
            J[0] = qy * ln2 - qz * ln1; // p x n, icp.hpp:105
            J[1] = qz * ln0 - qx * ln2;
            J[2] = qx * ln1 - qy * ln0;
            J[3] = ln0;
            J[4] = ln1;
            J[5] = ln2;
            const double e0 = lq0 - qx, e1 = lq1 - qy, e2 = lq2 - qz;
            const double bb = (e0 * ln0 + e1 * ln1) + e2 * ln2; // icp.hpp:116
            double *row = jrow[qi];
#if ICPMI_SMALL_ROBUST
            // the gate as below, then the weight of a kept row on its terms (icp_robust.h's contract): a dropped row leaves
            // a zero row with 0 in columns 28 and 29; with w == 1.0 every product is the gated kernel's
            const bool keep = (e0 * e0 + e1 * e1) + e2 * e2 <= g2;
            const double w = keep ? robust_weight(kind, ks, bb) : 0.0;
            row[28] = w;
            row[29] = keep ? 1.0 : 0.0;
            if (!keep) {
#pragma unroll
                for (int e = 0; e < 28; ++e) row[e] = 0.0;
            } else {
                double wJ[6];
#pragma unroll
                for (int r = 0; r < 6; ++r) wJ[r] = w * J[r];
                int o = 0;
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = r; c < 6; ++c) row[o++] = wJ[r] * J[c];
#pragma unroll
                for (int r = 0; r < 6; ++r) row[21 + r] = wJ[r] * bb;
                row[27] = (w * bb) * bb;
            }
#else
#if ICPMI_SMALL_GATED
            // the gate: a row whose winner is farther than sqrt(g2) -- or whose distance is a NaN -- leaves a zero row with
            // count 0, a kept row count 1; the rows and the order of additions are the ungated kernel's.  (The zero row IS
            // added, as +0.0, where k_reduce_gated adds nothing: x + 0.0 is x except for x = -0.0, so at most the sign of
            // a zero partial differs, and finish_sums adds every partial to an accumulator that starts at +0.0.)
            const bool keep = (e0 * e0 + e1 * e1) + e2 * e2 <= g2;
            row[28] = keep ? 1.0 : 0.0;
            if (!keep) {
#pragma unroll
                for (int e = 0; e < 28; ++e) row[e] = 0.0;
            } else {
#endif
            int o = 0;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = r; c < 6; ++c) row[o++] = J[r] * J[c];
#pragma unroll
            for (int r = 0; r < 6; ++r) row[21 + r] = J[r] * bb;
            row[27] = bb * bb;
#if ICPMI_SMALL_GATED
            }
#endif
#endif
#endif
        } else if (!valid && ql == 0) {
#pragma unroll
            for (int e = 0; e < ICPMI_SMALL_COLS; ++e) jrow[qi][e] = 0.0;
        }
    }
    __builtin_amdgcn_wave_barrier();
    // k_nn_resolve4<8>'s order: a wave's four rows, then the waves in order
    if (lane < ICPMI_SMALL_COLS)
        red[wave][lane] = ((jrow[wave * 4][lane] + jrow[wave * 4 + 1][lane]) + jrow[wave * 4 + 2][lane]) + jrow[wave * 4 + 3][lane];
    __syncthreads();
    if (threadIdx.x < ICPMI_SMALL_COLS) {
        const int e = threadIdx.x;
        double v = red[0][e];
#pragma unroll
        for (int w = 1; w < kSmallWaves; ++w) v += red[w][e];
        partials[(size_t)blockIdx.x * kSumsStride + e] = v;
    }
}
#undef ICPMI_SMALL_COLS
