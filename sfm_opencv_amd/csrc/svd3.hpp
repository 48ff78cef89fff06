// svd3.hpp -- the SVD of a 3 x 3 matrix by one-sided Jacobi rotations (Hestenes), one body for the host (sfmhip_pose_from_projection, twoview.hip)
// and the device (the decomposition of F in relpose.hip).  It finds a small singular value to its own precision where an eigen-solver on
// M^T M would square the ratio away.  Include it under `#pragma clang fp contract(off)`: sfmhip.h prescribes this arithmetic, operation by
// operation.  Every index below is a constant once the loops are unrolled, and what the order of the singular values decides at run time
// is picked with selects, so on the device the three matrices stay in registers.
#pragma once

namespace svd3 {

__host__ __device__ __forceinline__ double pick(int o, double x0, double x1, double x2) { return o == 0 ? x0 : o == 1 ? x1 : x2; }

// the determinant by the cofactors of column 0
__host__ __device__ __forceinline__ double det(const double (&m)[3][3])
{
    return m[0][0] * (m[1][1] * m[2][2] - m[2][1] * m[1][2]) - m[1][0] * (m[0][1] * m[2][2] - m[2][1] * m[0][2]) +
           m[2][0] * (m[0][1] * m[1][2] - m[1][1] * m[0][2]);
}

// M = u diag(s) v^T: at most 60 sweeps over the column pairs (0,1), (0,2), (1,2); a pair is skipped when its columns are orthogonal to
// 1e-16; s descending (the first of equals first); a column of u whose singular value is zero is zero; where s2 is not above 1e-15 s0
// (rank two) the third left vector completes the other two, with the sign of det v.
__host__ __device__ inline void jacobi(const double (&M)[3][3], double (&u)[3][3], double (&v)[3][3], double (&s)[3])
{
    double U[3][3], V[3][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) U[i][j] = M[i][j];
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                double a = 0, b = 0, c = 0;
#pragma unroll
                for (int i = 0; i < 3; ++i) { a += U[i][p] * U[i][p]; b += U[i][q] * U[i][q]; c += U[i][p] * U[i][q]; }
                if (c == 0.0 || fabs(c) <= 1e-16 * sqrt(a * b)) continue;
                rotated = true;
                const double zeta = (b - a) / (2.0 * c);
                const double tn = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double up = U[i][p], uq = U[i][q], vp = V[i][p], vq = V[i][q];
                    U[i][p] = cs * up - sn * uq; U[i][q] = sn * up + cs * uq;
                    V[i][p] = cs * vp - sn * vq; V[i][q] = sn * vp + cs * vq;
                }
            }
        if (!rotated) break;
    }
    double S[3];
    int ord[3] = { 0, 1, 2 };
#pragma unroll
    for (int j = 0; j < 3; ++j) S[j] = sqrt(U[0][j] * U[0][j] + U[1][j] * U[1][j] + U[2][j] * U[2][j]);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = a + 1; b < 3; ++b)
            if (pick(ord[b], S[0], S[1], S[2]) > pick(ord[a], S[0], S[1], S[2])) { const int o = ord[a]; ord[a] = ord[b]; ord[b] = o; }
#pragma unroll
    for (int j = 0; j < 3; ++j) {                                       // columns in descending order of the singular values
        const int o = ord[j];
        s[j] = pick(o, S[0], S[1], S[2]);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            u[i][j] = s[j] > 0.0 ? pick(o, U[i][0], U[i][1], U[i][2]) / s[j] : 0.0;
            v[i][j] = pick(o, V[i][0], V[i][1], V[i][2]);
        }
    }
    if (!(s[2] > 1e-15 * s[0])) {                                       // rank two: the third left vector completes the other two
        const double sgn = det(v) < 0 ? -1.0 : 1.0;
        u[0][2] = sgn * (u[1][0] * u[2][1] - u[2][0] * u[1][1]);
        u[1][2] = sgn * (u[2][0] * u[0][1] - u[0][0] * u[2][1]);
        u[2][2] = sgn * (u[0][0] * u[1][1] - u[1][0] * u[0][1]);
    }
}

}  // namespace svd3
