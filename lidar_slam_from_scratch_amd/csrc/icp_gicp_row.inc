// icp_gicp_row.inc -- the row arithmetic of plane-to-plane ICP (icp_gicp.h has the contract), as text: k_reduce_gicp
// includes it in its loop body, so the arithmetic sits in the kernel itself (kernels.h: bodies inlined from a device
// function had operands commuted), and tests/cpp/gicp_row_host.cpp includes the same text for the host compiler, which
// tests/test_gicp_header.py holds to scripts/gicp_ref.py's bits.  Unfused fp64 (-ffp-contract=off on both sides).
//
// ICPMI_GICP_PART 1: the source normal in the target frame.  In: R00..R22 (rotation of IcpState::total), s0, s1, s2.
//                    Out: m0, m1, m2.
// ICPMI_GICP_PART 2: a kept row's 29 columns.  In: p0..p2 (the moved source row), e0..e2 (q - p), n0..n2, m0..m2, c, kappa.
//                    Out: ICPMI_GICP_COL(k, value) once for every column k = 0..28, in ascending order.
#if ICPMI_GICP_PART == 1
        const double m0 = (R00 * s0 + R01 * s1) + R02 * s2;
        const double m1 = (R10 * s0 + R11 * s1) + R12 * s2;
        const double m2 = (R20 * s0 + R21 * s1) + R22 * s2;
#elif ICPMI_GICP_PART == 2
        // S = 2 I - c (n n^T + m m^T): the two plane-regularised covariances I - c n n^T and I - c m m^T, added
        const double S00 = 2.0 - c * (n0 * n0 + m0 * m0);
        const double S01 = 0.0 - c * (n0 * n1 + m0 * m1);
        const double S02 = 0.0 - c * (n0 * n2 + m0 * m2);
        const double S11 = 2.0 - c * (n1 * n1 + m1 * m1);
        const double S12 = 0.0 - c * (n1 * n2 + m1 * m2);
        const double S22 = 2.0 - c * (n2 * n2 + m2 * m2);
        // M = S^-1 by cofactors: one division
        const double C00 = S11 * S22 - S12 * S12;
        const double C01 = S02 * S12 - S01 * S22;
        const double C02 = S01 * S12 - S02 * S11;
        const double C11 = S00 * S22 - S02 * S02;
        const double C12 = S01 * S02 - S00 * S12;
        const double C22 = S00 * S11 - S01 * S01;
        const double det = (S00 * C00 + S01 * C01) + S02 * C02;
        const double r = 1.0 / det;
        const double M00 = C00 * r, M01 = C01 * r, M02 = C02 * r, M11 = C11 * r, M12 = C12 * r, M22 = C22 * r;
        // u = M e
        const double u0 = (M00 * e0 + M01 * e1) + M02 * e2;
        const double u1 = (M01 * e0 + M11 * e1) + M12 * e2;
        const double u2 = (M02 * e0 + M12 * e1) + M22 * e2;
        // B = [p]x M, the rotation rows against the translation columns of A^T M A: B_rc = (p x M_c)_r, M_c = column c of M
        const double B00 = p1 * M02 - p2 * M01, B01 = p1 * M12 - p2 * M11, B02 = p1 * M22 - p2 * M12;
        const double B10 = p2 * M00 - p0 * M02, B11 = p2 * M01 - p0 * M12, B12 = p2 * M02 - p0 * M22;
        const double B20 = p0 * M01 - p1 * M00, B21 = p0 * M11 - p1 * M01, B22 = p0 * M12 - p1 * M02;
        // G = B (-[p]x), the rotation block (its upper triangle): G_r0 = B_r2 p1 - B_r1 p2, G_r1 = B_r0 p2 - B_r2 p0,
        // G_r2 = B_r1 p0 - B_r0 p1
        ICPMI_GICP_COL(0, B02 * p1 - B01 * p2)
        ICPMI_GICP_COL(1, B00 * p2 - B02 * p0)
        ICPMI_GICP_COL(2, B01 * p0 - B00 * p1)
        ICPMI_GICP_COL(3, B00)
        ICPMI_GICP_COL(4, B01)
        ICPMI_GICP_COL(5, B02)
        ICPMI_GICP_COL(6, B10 * p2 - B12 * p0)
        ICPMI_GICP_COL(7, B11 * p0 - B10 * p1)
        ICPMI_GICP_COL(8, B10)
        ICPMI_GICP_COL(9, B11)
        ICPMI_GICP_COL(10, B12)
        ICPMI_GICP_COL(11, B21 * p0 - B20 * p1)
        ICPMI_GICP_COL(12, B20)
        ICPMI_GICP_COL(13, B21)
        ICPMI_GICP_COL(14, B22)
        ICPMI_GICP_COL(15, M00)
        ICPMI_GICP_COL(16, M01)
        ICPMI_GICP_COL(17, M02)
        ICPMI_GICP_COL(18, M11)
        ICPMI_GICP_COL(19, M12)
        ICPMI_GICP_COL(20, M22)
        // A^T u = (p x u, u)
        ICPMI_GICP_COL(21, p1 * u2 - p2 * u1)
        ICPMI_GICP_COL(22, p2 * u0 - p0 * u2)
        ICPMI_GICP_COL(23, p0 * u1 - p1 * u0)
        ICPMI_GICP_COL(24, u0)
        ICPMI_GICP_COL(25, u1)
        ICPMI_GICP_COL(26, u2)
        ICPMI_GICP_COL(27, kappa * ((e0 * u0 + e1 * u1) + e2 * u2))
        ICPMI_GICP_COL(28, 1.0)
#else
#error "ICPMI_GICP_PART is 1 or 2"
#endif
