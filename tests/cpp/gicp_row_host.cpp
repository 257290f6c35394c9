// The row arithmetic of plane-to-plane ICP for the host compiler: the text k_reduce_gicp includes in its loop body
// (csrc/icp_gicp_row.inc), around which this file only declares the inputs and stores the outputs.  Built by
// tests/test_gicp_header.py with -ffp-contract=off as a shared object and compared bit for bit with scripts/gicp_ref.py.
// (Same text, two compilers: that the device compiler keeps the order too is what tests/test_gpu_gicp.py's parity shows.)

// total: 16 doubles, row-major (IcpState::total); s: the source row's normal -> m[3]
extern "C" void gicp_rotate_normal(const double *total, const double *s, double *m_out)
{
    const double R00 = total[0], R01 = total[1], R02 = total[2];
    const double R10 = total[4], R11 = total[5], R12 = total[6];
    const double R20 = total[8], R21 = total[9], R22 = total[10];
    for (int i = 0; i < 1; ++i) {
        const double s0 = s[0], s1 = s[1], s2 = s[2];
#define ICPMI_GICP_PART 1
#include "../../lidar_slam_from_scratch_amd/csrc/icp_gicp_row.inc"
#undef ICPMI_GICP_PART
        m_out[0] = m0, m_out[1] = m1, m_out[2] = m2;
    }
}

// rows: `count` rows of p, q, n, m (3 doubles each) -> cols[count][29]
extern "C" void gicp_row_columns(const double *p, const double *q, const double *n, const double *m, long count, double c,
                                 double kappa, double *cols)
{
    for (long i = 0; i < count; ++i) {
        const double p0 = p[3 * i], p1 = p[3 * i + 1], p2 = p[3 * i + 2];
        const double q0 = q[3 * i], q1 = q[3 * i + 1], q2 = q[3 * i + 2];
        const double n0 = n[3 * i], n1 = n[3 * i + 1], n2 = n[3 * i + 2];
        const double m0 = m[3 * i], m1 = m[3 * i + 1], m2 = m[3 * i + 2];
        const double e0 = q0 - p0, e1 = q1 - p1, e2 = q2 - p2;
        double *acc = cols + 29 * i;
#define ICPMI_GICP_PART 2
#define ICPMI_GICP_COL(k, value) acc[k] = (value);
#include "../../lidar_slam_from_scratch_amd/csrc/icp_gicp_row.inc"
#undef ICPMI_GICP_COL
#undef ICPMI_GICP_PART
    }
}
